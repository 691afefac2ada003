"""The streaming glue kernels (rbx_cross_fwd / _bwd, rbx_rowscale, rbx_rowscale_seq, rbx_seq_colsum, rbx_sum_prefix,
rbx_scale_by_scalar) and xDeepFM's CIN outer product (rbx_cin_outer_fwd / _bwd) against the float64 restatements of
oracle/glue64.py at every form they dispatch, element by element: |got - want| <= C eps32 A + tiny with the constants of that
file's docstring, and ``torch.equal`` where the result is one product or a copy.  Every comparison goes through ``check`` /
``exact``; outputs and workspaces of direct C-ABI calls start NaN-filled, operands are views of NaN-filled buffers (four
spare floats behind, ``offset`` floats in front), and whatever lies outside the documented output must still be NaN.

Forms, read from the dispatch code (kCUs = 256 in rbx_internal.h; every grid-stride kernel has 256 threads per workgroup):
  cross_fwd       cross_fwd_kernel<true> (one float4 per thread) when dim % 4 == 0 and x0, xi, h, out are 16-byte aligned
                  (bias is read element by element); else cross_fwd_kernel<false>.  Grid capped at kCUs * 16 workgroups:
                  the second trip starts past 1 048 576 float4s (4100 x 1024) or elements.
  cross_bwd       cross_bwd_kernel<64> always: a 64-lane group per row, 4 rows per workgroup, lane c % 64 walks the row;
                  h_cols == 1 ends in group_sum<64> (dim == 1 is this form: h_cols == 1 == dim).  Grid capped at
                  kCUs * 16 workgroups: the second trip starts past 16 384 rows.
  rowscale(_seq)  rowscale_kernel<true> (float4) when dim % 4 == 0 and x, add, out are 16-byte aligned, else
                  rowscale_kernel<false>: four flat elements per thread, which straddle rows whenever dim % 4 != 0.
                  Grid capped at kCUs * 32: the second trip starts past 8 388 608 elements (131 080 x 64).
  seq_colsum      seq_colsum_partial_kernel<4> when dim % 4 == 0 and g is 16-byte aligned, else <1>; one partial per 32
                  sequences, 8 rows in flight; seq_colsum_final_kernel adds the partials 8 at a time plus a remainder.
  sum_prefix      sum_prefix_kernel<true> when base, a, b, out are 16-byte aligned, prefix_cols % 4 == 0, every stride is a
                  multiple of 4 and out_stride, base_stride >= cols rounded up to 4; else sum_prefix_kernel<false>.
                  Grid capped at kCUs * 16: the second trip starts past 1 048 576 float4s (2500 x 1677).  In every form only
                  out[r, 0 .. cols) is written.  The 64-bit row division (rows * per_row >= 2^32) is out of reach of a
                  test: it needs 16 GiB per operand.
  scale_by_scalar one kernel; grid capped at kCUs * 8: the second trip starts past 524 288 elements.
  cin_outer       one workgroup per sample, LDS (F + M) D floats forward, + F M + F D backward; above 64 KB the entry point
                  raises the kernel's dynamic LDS limit first, above 160 KB it refuses (RBX_ERR_UNSUPPORTED).  The backward's
                  t loop takes a second trip when F + M > 256.
      (B, F, D, M)         forward LDS    backward LDS
      (2, 39, 16, 24)      4 KB           10 KB
      (2, 39, 40, 200)     37 KB          74 KB  (raised)
      (2, 39, 64, 256)     74 KB (raised) 123 KB (raised)
      (2, 130, 8, 130)     8 KB           78 KB  (raised), F + M = 260
      (1, 1, 13654, 1)     107 KB         160 KB + 12 bytes: the smallest backward that is refused
      (1, 1, 20481, 1)     160 KB + 8 bytes: the smallest forward that is refused

Worst err / bound observed on the MI355X (the ledger of conftest._note has every label):
  op                         worst over every form and input
  cross forward              out 0.015 (<true> 0.015, <false> 0.014, past the grid cap 0.015)
  cross backward             dh row sum 0.017 (past the grid cap); dx0 and the element-wise dh: equal
  ops.cross                  out 0.012   dh row sum 0.011   dbias 0.0094   dx0, dxi: equal
  CrossNet / CrossNetV2      2.2e-6 (output, dx) and 3.2e-6 (parameter gradients) absolute, against f32_tol >= 2e-5
  rowscale                   0.015 (<false> at (4096, 7), <true> past the grid cap); without add at alpha = 1: equal
  rowscale_seq               0.015
  ops.row_scale, offset view out 0.013   dx 0.0078   dadd: equal
  ops.sasrec_input           out, de, dpos 0.019 (0.016 on the offset views)
  seq_colsum                 <4> 0.034   <1> 0.027 (0.027 forced at dim 64); two runs bit-equal; batch 0: zero
  sum_prefix                 0.016 (three operands; two: 0.0078); one operand or none: equal; past the grid cap 0.016
  scale_by_scalar            equal, and so is dL/dlogit of (loss * 0.37)
  cin_outer                  z: equal   dx0 0.039 (130, 8, 130)   dxk 0.053 (39, 40, 200)
  split_last                 values and dx: equal
  180 cases, 4.7 s for the file (the slowest case 0.84 s).  Nothing is above 0.5.

Mutation check (scratch builds, not committed): two single-line faults, each linked into a library of its own.
  (a) seq_colsum_final_kernel drops the remainder loop after its 8-wide trips.  tests/test_gpu_matching.py and
      tests/test_gpu_ranking.py as they were (the two files that held this family's tests): 255 of 261 pass; the six that
      notice are test_sasrec_input_reads_position_rows_in_place (all four shapes), test_sasrec_golden and
      test_sasrec_longer_than_the_matrix_core_kernels_take.  This file: 17 failed -- seq_colsum_every_batch at 1, 7, 8, 31,
      32, 33, 257 and 290 (every count of partials that is no multiple of 8; 255 and 256 have exactly 8 and pass), the three
      forced <1> cases and the six ops.sasrec_input cases.
  (b) cin_outer_bwd_kernel's t loop does not advance past blockDim.x (an ``if`` in its place).  The same two earlier files:
      261 of 261 pass -- nothing earlier had F + M > 256.  This file: 6 failed, exactly the shapes with F + M > 256, both
      input kinds: cin_every_shape at (2, 39, 64, 256), (2, 130, 8, 130) and (2, 130, 8, None)."""
import ctypes

import pytest
import torch

from conftest import _note, assert_close
from oracle import glue64 as G
from test_glue64_restatement import (CIN_SHAPES, COLSUM_BATCHES, CROSS_DIMS, CROSS_ROWS, PREFIX_ROWS, PREFIX_SHAPES,
                                     ROWSCALE_SHAPES, SCALAR_NS, SEQ_SHAPES, SUBSETS, cin_case, cross_case, prefix_case,
                                     rowscale_case, seq_case)
from test_gpu_dense_routes import f32_tol
from test_interact64_restatement import randn

pytestmark = pytest.mark.gpu

EPS32, TINY = G.EPS32, G.TINY
NAN = float("nan")
K_CUS = 256                     # rbx_internal.h: kCUs
OK, INVALID, WORKSPACE, UNSUPPORTED = 0, -1, -3, -4


def check(label, got, want, A, C):
    """THE comparison: every element within C eps32 A + tiny; notes the worst err / bound under ``label``."""
    got = got.detach().double().cpu().reshape(want.shape)
    assert not bool(torch.isnan(got).any()), "%s: %d elements were never written" % (label, int(torch.isnan(got).sum()))
    bound = C * EPS32 * A + TINY
    err = (got - want).abs()
    r = float((err / bound).max()) if err.numel() else 0.0
    _note("%s (err / bound)" % label, r, 1.0)
    print("%s: %.3g" % (label, r))
    assert bool((err <= bound).all()), "%s: %.3g x the bound (%d of %d elements)" % (label, r, int((err > bound).sum()), err.numel())


def exact(label, got, want):
    """One product, a copy or a zero: the float32 rounding of the float64 value, bit for bit (torch.equal)."""
    got = got.detach().cpu().reshape(want.shape)
    assert not bool(torch.isnan(got).any()), "%s: %d elements were never written" % (label, int(torch.isnan(got).sum()))
    same = torch.equal(got, want.float())
    _note("%s (unequal elements)" % label, float((got != want.float()).sum()), 0.0)
    assert same, "%s: %d of %d elements differ" % (label, int((got != want.float()).sum()), got.numel())


class Placed(object):
    """[rows, cols] as a view (row stride ``stride``, ``offset`` floats into the storage) of a NaN-filled buffer with four
    spare floats behind; ``untouched()``: everything outside the view is still NaN."""

    def __init__(self, rows, cols, data=None, stride=None, offset=0):
        stride = cols if stride is None else stride
        n = offset + rows * stride + 4
        self.buf = torch.full((n,), NAN, dtype=torch.float32, device="cuda")
        self.view = self.buf.as_strided((rows, cols), (stride, 1), offset)
        self.stride = stride
        if data is not None:
            self.view.copy_(data.reshape(rows, cols))
        self.mask = torch.ones(n, dtype=torch.bool, device="cuda")
        self.mask.as_strided((rows, cols), (stride, 1), offset).fill_(False)

    @property
    def ptr(self):
        return ctypes.c_void_p(self.view.data_ptr())

    def untouched(self):
        return bool(torch.isnan(self.buf[self.mask]).all())

    def all_nan(self):
        return bool(torch.isnan(self.buf).all())


def place(t, offset=0):
    """A contiguous tensor of any rank, placed: one row."""
    return Placed(1, t.numel(), t, offset=offset) if t is not None else None


def p_(x):
    return x.ptr if x is not None else None


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def lib():
    from recbox_amd._lib import lib as the_lib
    return the_lib


# ---- cross on the C ABI ---------------------------------------------------------------------------------------------------
def run_cross(label, case, offset=0, skip_dx0=False):
    x0, xi, h, bias, g = case
    rows, dim = x0.shape
    hc = h.shape[1]
    px0, pxi, ph, pb, pg = place(x0, offset), place(xi, offset), place(h, offset), place(bias, 1), place(g, offset)
    out = Placed(1, rows * dim, offset=offset)
    assert lib().rbx_cross_fwd(px0.ptr, pxi.ptr, ph.ptr, p_(pb), rows, dim, hc, out.ptr, stream()) == OK
    dx0, dh = Placed(1, rows * dim, offset=offset), Placed(1, rows * hc, offset=offset)
    assert lib().rbx_cross_bwd(px0.ptr, ph.ptr, pg.ptr, rows, dim, hc, None if skip_dx0 else dx0.ptr, dh.ptr, stream()) == OK
    torch.cuda.synchronize()
    want, A = G.cross_fwd(x0, xi, h, bias)
    check(label + " out", out.view, want, A, G.c_cross_fwd())
    (wdx0, _), (wdh, a_dh) = G.cross_bwd(x0, h, g)
    if skip_dx0:
        assert dx0.all_nan()
    else:
        exact(label + " dx0", dx0.view, wdx0)
    if hc == 1 and dim > 1:
        check(label + " dh row sum", dh.view, wdh, a_dh, G.c_cross_dh(dim))
    else:
        exact(label + " dh", dh.view, wdh)
    assert out.untouched() and dx0.untouched() and dh.untouched()


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("broadcast", [False, True])
@pytest.mark.parametrize("dim", CROSS_DIMS)
def test_cross_every_form(dim, broadcast, offset):
    """offset 1: every tensor one float into its storage, which is the scalar forward at the float4 dims."""
    for rows in CROSS_ROWS:
        for bias in (True, False):
            case = cross_case(rows, dim, 1 if broadcast else dim, bias, seed=offset)
            form = "cross<%s> dim %d h_cols %s" % ("T" if dim % 4 == 0 and not offset else "F", dim, "1" if broadcast else "dim")
            run_cross(form, case, offset)


@pytest.mark.parametrize("dim", [1, 3, 63, 65, 200, 256])
def test_cross_row_sum_one_signed_and_without_dx0(dim):
    run_cross("cross dim %d one-signed" % dim, cross_case(5, dim, 1, True, seed=3, kind="one_signed"))
    run_cross("cross dim %d no dx0" % dim, cross_case(5, dim, 1, False, seed=4, kind="one_signed"), skip_dx0=True)
    run_cross("cross dim %d h dim no dx0" % dim, cross_case(5, dim, dim, False, seed=4), skip_dx0=True)


def test_cross_empty_batch_and_the_h_cols_refusal():
    assert lib().rbx_cross_fwd(None, None, None, None, 0, 8, 8, None, stream()) == OK
    assert lib().rbx_cross_bwd(None, None, None, 0, 8, 1, None, None, stream()) == OK
    x0, xi, h, bias, g = cross_case(5, 8, 2, True)
    t = [place(v) for v in (x0, xi, h, bias, g)]
    out, dx0, dh = Placed(5, 8), Placed(5, 8), Placed(5, 2)
    assert lib().rbx_cross_fwd(t[0].ptr, t[1].ptr, t[2].ptr, t[3].ptr, 5, 8, 2, out.ptr, stream()) == INVALID
    assert lib().rbx_cross_bwd(t[0].ptr, t[2].ptr, t[4].ptr, 5, 8, 2, dx0.ptr, dh.ptr, stream()) == INVALID
    assert lib().rbx_cross_fwd(t[0].ptr, t[1].ptr, t[2].ptr, t[3].ptr, 5, 0, 1, out.ptr, stream()) == INVALID
    torch.cuda.synchronize()
    assert out.all_nan() and dx0.all_nan() and dh.all_nan()


def test_cross_past_the_grid_caps():
    """Forward: 4100 x 1024 is 1 049 600 float4s, 1024 past kCUs * 16 * 256.  Backward: 16 389 rows, 5 past kCUs * 16 * 4."""
    rows, dim = 4100, 1024
    assert rows * dim // 4 > K_CUS * 16 * 256
    x0, xi, h, bias, _ = cross_case(rows, dim, 1, True, seed=5)
    px0, pxi, ph, pb, out = place(x0), place(xi), place(h), place(bias), Placed(1, rows * dim)
    assert lib().rbx_cross_fwd(px0.ptr, pxi.ptr, ph.ptr, pb.ptr, rows, dim, 1, out.ptr, stream()) == OK
    torch.cuda.synchronize()
    want, A = G.cross_fwd(x0, xi, h, bias)
    check("cross<T> forward past the grid cap", out.view, want, A, G.c_cross_fwd())
    assert out.untouched()
    rows = K_CUS * 16 * 4 + 5
    run_cross("cross backward past the grid cap", cross_case(rows, 4, 1, False, seed=6))
    run_cross("cross backward past the grid cap h dim", cross_case(rows, 4, 4, False, seed=6))


@pytest.mark.parametrize("broadcast", [False, True])
@pytest.mark.parametrize("rows,dim", [(257, 8), (5, 100), (37, 3)])
def test_ops_cross_gradients_on_non_contiguous_inputs(rows, dim, broadcast):
    """Through ops.cross: x0 and xi arrive transposed, h as every other column of a wider tensor; dxi is the upstream
    gradient itself and dbias its column sum."""
    from recbox_amd import ops
    x0, xi, h, bias, g = cross_case(rows, dim, 1 if broadcast else dim, True, seed=7)
    l0 = x0.t().contiguous().cuda().requires_grad_(True)
    li = xi.t().contiguous().cuda().requires_grad_(True)
    lh = torch.stack([h, h], dim=2).cuda().requires_grad_(True)
    lb = bias.cuda().requires_grad_(True)
    a0, ai, ah = l0.t(), li.t(), lh[:, :, 1]
    assert not a0.is_contiguous() and (not ah.is_contiguous() or rows == 1)
    out = ops.cross(a0, ai, ah, lb)
    out.backward(g.cuda())
    torch.cuda.synchronize()
    want, A = G.cross_fwd(x0, xi, h, bias)
    check("ops.cross out", out, want, A, G.c_cross_fwd())
    (wdx0, _), (wdh, a_dh) = G.cross_bwd(x0, h, g)
    exact("ops.cross dx0", l0.grad.t(), wdx0)
    exact("ops.cross dxi", li.grad.t(), g.double())
    if broadcast and dim > 1:
        check("ops.cross dh row sum", lh.grad[:, :, 1], wdh, a_dh, G.c_cross_dh(dim))
    else:
        exact("ops.cross dh", lh.grad[:, :, 1], wdh)
    assert int(lh.grad[:, :, 0].count_nonzero()) == 0
    # torch's own column sum, whatever its order: the sequential bound of `rows` terms
    check("ops.cross dbias", lb.grad, g.double().sum(0), g.double().abs().sum(0), max(G.C_BOUND, rows + 2))


@pytest.mark.parametrize("which", ["CrossNet", "CrossNetV2"])
@pytest.mark.parametrize("rows,dim", [(37, 24), (5, 7)])
def test_cross_layers_two_deep_vs_float64(which, rows, dim):
    """Two stacked layers: the output and every parameter gradient against float64 torch on the reference's expressions
    (cross_net.py:34-59), at the float32 tolerance of the GEMM tests (f32_tol of the reduction length)."""
    from recbox_amd.ranking.pytorch.layers import interactions as I
    torch.manual_seed(rows + dim)
    net = getattr(I, which)(dim, 2)
    with torch.no_grad():
        for i, p in enumerate(net.parameters()):
            p.copy_(randn(p.shape, 20 + i) * 0.3)
    x = (randn((rows, dim), 11) * 0.5)
    R = randn((rows, dim), 12)
    params = dict((n, p.detach().double().requires_grad_(True)) for n, p in net.named_parameters())
    xr = x.double().requires_grad_(True)
    xi = xr
    for i in range(2):
        if which == "CrossNet":
            w, b = params["cross_net.%d.weight.weight" % i], params["cross_net.%d.bias" % i]
            xi = xi + (xi @ w.t()) * xr + b
        else:
            w, b = params["cross_layers.%d.weight" % i], params["cross_layers.%d.bias" % i]
            xi = xi + xr * (xi @ w.t() + b)
    (xi * R.double()).sum().backward()
    net.cuda()
    xc = x.cuda().requires_grad_(True)
    out = net(xc)
    (out * R.cuda()).sum().backward()
    torch.cuda.synchronize()
    assert_close(out, xi.detach(), f32_tol(dim), which + " out")
    assert_close(xc.grad, xr.grad, f32_tol(dim), which + " dx")
    for n, p in net.named_parameters():
        assert_close(p.grad, params[n].grad, f32_tol(rows), which + " grad " + n)


# ---- rowscale / rowscale_seq ----------------------------------------------------------------------------------------------
def run_rowscale(label, x, add, s, alpha, offset=0, seq=None):
    """seq: (B, L) -- ``add`` is then the [L, D] block of rbx_rowscale_seq."""
    dim = x.shape[-1]
    rows = x.numel() // dim
    px, pa, ps = place(x, offset), place(add, offset), place(s)
    out = Placed(1, rows * dim, offset=offset)
    if seq is None:
        rc = lib().rbx_rowscale(px.ptr, p_(pa), ps.ptr, rows, dim, alpha, out.ptr, stream())
        want, A = G.rowscale(x, add, s, alpha)
    else:
        rc = lib().rbx_rowscale_seq(px.ptr, pa.ptr, seq[1], ps.ptr, rows, dim, alpha, out.ptr, stream())
        want, A = G.rowscale_seq(x, add, s, alpha)
    assert rc == OK
    torch.cuda.synchronize()
    if add is None and alpha == 1.0:
        exact(label, out.view, want)
    else:
        check(label, out.view, want, A, G.c_rowscale())
    assert out.untouched()


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("rows,dim", ROWSCALE_SHAPES)
def test_rowscale_every_shape(rows, dim, offset):
    """(3, 7): the row boundaries fall inside a thread's four elements and the total is no multiple of 4.  offset 1 at
    dim % 4 == 0: the scalar form on a misaligned tensor (it used to be refused)."""
    form = "rowscale<%s> (%d, %d)" % ("T" if dim % 4 == 0 and not offset else "F", rows, dim)
    for with_add in (True, False):
        for alpha in (1.0, 8.0):
            x, add, s, _ = rowscale_case(rows, dim, with_add, seed=offset, kind="one_signed" if alpha == 8.0 and not with_add else "randn")
            run_rowscale("%s add %d alpha %g" % (form, with_add, alpha), x, add, s, alpha, offset)


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("B,L,D", SEQ_SHAPES)
def test_rowscale_seq_every_shape(B, L, D, offset):
    form = "rowscale_seq<%s> (%d, %d, %d)" % ("T" if D % 4 == 0 and not offset else "F", B, L, D)
    for alpha in (1.0, 8.0):
        x, pos, keep, _ = seq_case(B, L, D, seed=offset)
        run_rowscale("%s alpha %g" % (form, alpha), x, pos, keep, alpha, offset, seq=(B, L))


def test_rowscale_refusals():
    x, pos, keep, _ = seq_case(3, 5, 4)
    px, pp, ps, out = place(x), place(pos), place(keep), Placed(15, 4)
    assert lib().rbx_rowscale_seq(px.ptr, pp.ptr, 4, ps.ptr, 15, 4, 1.0, out.ptr, stream()) == INVALID       # 15 % 4 != 0
    assert lib().rbx_rowscale_seq(px.ptr, pp.ptr, 0, ps.ptr, 15, 4, 1.0, out.ptr, stream()) == INVALID
    assert lib().rbx_rowscale_seq(px.ptr, None, 5, ps.ptr, 15, 4, 1.0, out.ptr, stream()) == INVALID
    assert lib().rbx_rowscale(px.ptr, None, None, 15, 4, 1.0, out.ptr, stream()) == INVALID
    assert lib().rbx_rowscale(None, None, None, 0, 4, 1.0, None, stream()) == OK
    torch.cuda.synchronize()
    assert out.all_nan()


def test_rowscale_past_the_grid_cap():
    rows, dim = 131080, 64
    assert rows * dim > K_CUS * 32 * 256 * 4
    x, add, s, _ = rowscale_case(rows, dim, True, seed=2)
    run_rowscale("rowscale<T> past the grid cap", x, add, s, 8.0)


@pytest.mark.parametrize("shape", [(9, 4), (3, 5, 64), (5, 6)])
def test_ops_row_scale_on_a_view_one_float_into_its_storage(shape):
    """ops.row_scale keeps a contiguous view where it is: at dim % 4 == 0 the kernel's scalar form computes it, forward and
    backward (the upstream gradient is such a view as well)."""
    from recbox_amd import ops
    rows, dim = shape[0] * (shape[1] if len(shape) == 3 else 1), shape[-1]
    x, add, s, g = rowscale_case(rows, dim, True, seed=8)
    px, pa, pg = place(x, 1), place(add, 1), place(g, 1)
    xv = px.view.view(shape).requires_grad_(True)
    av = pa.view.view(shape).requires_grad_(True)
    assert xv.is_contiguous() and xv.data_ptr() % 16 == 4
    out = ops.row_scale(xv, s.cuda().view(shape[:-1]), add=av, alpha=8.0)
    out.backward(pg.view.view(shape))
    torch.cuda.synchronize()
    want, A = G.rowscale(x, add, s, 8.0)
    check("ops.row_scale offset view %s" % (shape,), out, want, A, G.c_rowscale())
    wdx, a_dx = G.rowscale(g, None, s, 8.0)
    check("ops.row_scale offset view %s dx" % (shape,), xv.grad, wdx, a_dx, G.c_rowscale())
    exact("ops.row_scale offset view %s dadd" % (shape,), av.grad, G.rowscale(g, None, s, 1.0)[0])


# ---- seq_colsum -----------------------------------------------------------------------------------------------------------
def run_colsum(label, g, keep, offset=0, ws_nan=True):
    B, L, D = g.shape
    pg, ps = place(g, offset), place(keep)
    out = Placed(L, D)
    nbytes = lib().rbx_seq_colsum_workspace_size(B, L, D)
    assert nbytes == -(-B // 32) * L * D * 4
    ws = torch.full((nbytes // 4 + 4,), NAN, device="cuda")
    outs = []
    for _ in range(2):
        out.view.fill_(NAN)
        ws.fill_(NAN)
        assert lib().rbx_seq_colsum(pg.ptr, ps.ptr, B, L, D, out.ptr, ctypes.c_void_p(ws.data_ptr()), nbytes, stream()) == OK
        torch.cuda.synchronize()
        outs.append(out.view.clone())
    want, A = G.seq_colsum(g, keep)
    check(label, outs[0], want, A, G.c_colsum(B))
    assert torch.equal(outs[0], outs[1]), label + ": two runs differ"
    assert out.untouched() and bool(torch.isnan(ws[nbytes // 4:]).all())


@pytest.mark.parametrize("batch", COLSUM_BATCHES)
def test_seq_colsum_every_batch(batch):
    """33 and 257: a last block of one sequence (seven clamped rows with scale 0); 290: ten partials -- one 8-wide trip of
    the final kernel and a remainder of two -- and a last block of 2.  L = 200 at dim 64 for 7, 33 and 290 sequences."""
    shapes = [(L, D) for L in (1, 5) for D in (4, 6, 64)] + ([(200, 64)] if batch in (7, 33, 290) else [])
    for i, (L, D) in enumerate(shapes):
        _, _, keep, g = seq_case(batch, L, D, seed=1, kind="one_signed" if i % 2 else "randn")
        run_colsum("seq_colsum<%d> B %d L %d D %d" % (4 if D % 4 == 0 else 1, batch, L, D), g, keep)


@pytest.mark.parametrize("batch", [7, 33, 290])
def test_seq_colsum_scalar_form_at_dim_64(batch):
    _, _, keep, g = seq_case(batch, 5, 64, seed=2, kind="one_signed")
    run_colsum("seq_colsum<1> forced at D 64, B %d" % batch, g, keep, offset=1)


def test_seq_colsum_empty_batch_and_the_workspace_refusal():
    out = Placed(5, 6)
    assert lib().rbx_seq_colsum(None, None, 0, 5, 6, out.ptr, None, 0, stream()) == OK
    torch.cuda.synchronize()
    exact("seq_colsum empty batch", out.view, torch.zeros(5, 6, dtype=torch.float64))
    assert out.untouched()
    _, _, keep, g = seq_case(33, 5, 6)
    pg, ps = place(g), place(keep)
    out = Placed(5, 6)
    nbytes = lib().rbx_seq_colsum_workspace_size(33, 5, 6)
    ws = torch.full((nbytes // 4,), NAN, device="cuda")
    wp = ctypes.c_void_p(ws.data_ptr())
    assert lib().rbx_seq_colsum(pg.ptr, ps.ptr, 33, 5, 6, out.ptr, None, nbytes, stream()) == WORKSPACE
    assert lib().rbx_seq_colsum(pg.ptr, ps.ptr, 33, 5, 6, out.ptr, wp, nbytes - 1, stream()) == WORKSPACE
    assert lib().rbx_seq_colsum(pg.ptr, ps.ptr, 33, 0, 6, out.ptr, wp, nbytes, stream()) == INVALID
    torch.cuda.synchronize()
    assert out.all_nan() and bool(torch.isnan(ws).all())
    assert lib().rbx_seq_colsum_workspace_size(0, 5, 6) == 0


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("B,L,D", [(3, 5, 7), (33, 5, 64), (290, 3, 4)])
def test_ops_sasrec_input_end_to_end(B, L, D, offset):
    """Forward, de and dpos through ops.sasrec_input; offset 1: e and the gradient one float into their storage."""
    from recbox_amd import ops
    x, pos, keep, g = seq_case(B, L, D, seed=9)
    alpha = float(D) ** 0.5
    px, pg = place(x, offset), place(g, offset)
    e = px.view.view(B, L, D).requires_grad_(True)
    table = torch.cat([pos, randn((2, D), 1)]).cuda().requires_grad_(True)
    out = ops.sasrec_input(e, table[:L], keep.cuda(), alpha=alpha)
    out.backward(pg.view.view(B, L, D))
    torch.cuda.synchronize()
    want, A = G.rowscale_seq(x, pos, keep, alpha)
    check("ops.sasrec_input out offset %d" % offset, out, want, A, G.c_rowscale())
    (de, a_de), (dpos, a_dpos) = G.sasrec_input_bwd(g, keep, alpha)
    check("ops.sasrec_input de offset %d" % offset, e.grad, de, a_de, G.c_rowscale())
    check("ops.sasrec_input dpos offset %d" % offset, table.grad[:L], dpos, a_dpos, G.c_colsum(B))
    assert int(table.grad[L:].count_nonzero()) == 0


# ---- sum_prefix -----------------------------------------------------------------------------------------------------------
def strides_of(kind, cols, prefix):
    """(out / base / b row stride, a row stride)."""
    padded = (cols + 3) // 4 * 4
    whole = {"exact": cols, "padded": padded, "wider": padded + 4, "odd": padded + 1}[kind]
    return whole, (prefix if kind in ("exact", "padded") else whole)


def run_prefix(label, rows, cols, prefix, kind, used, case=None, offset=0):
    base, a, b = case if case is not None else prefix_case(rows, cols, prefix)
    whole, a_stride = strides_of(kind, cols, prefix)
    pb = Placed(rows, cols, base, stride=whole, offset=offset) if used[0] else None
    pa = Placed(rows, prefix, a, stride=a_stride, offset=offset) if used[1] else None
    pc = Placed(rows, prefix, b, stride=whole, offset=offset) if used[2] else None
    out = Placed(rows, cols, stride=whole, offset=offset)
    rc = lib().rbx_sum_prefix(p_(pb), whole if pb else 0, p_(pa), a_stride if pa else 0, p_(pc), whole if pc else 0, rows, cols,
                              prefix, out.ptr, whole, stream())
    assert rc == OK
    torch.cuda.synchronize()
    want, A = G.sum_prefix(base if used[0] else None, a if used[1] else None, b if used[2] else None, rows, cols, prefix)
    n_ops = used[0] + (used[1] + used[2] if prefix else 0)
    if n_ops <= 1:
        exact(label, out.view, want)
    else:
        check(label, out.view, want, A, G.c_sum_prefix())
    assert out.untouched(), label + ": columns at or beyond `cols` were written"


@pytest.mark.parametrize("kind", ["exact", "padded", "wider", "odd"])
@pytest.mark.parametrize("cols,prefix", PREFIX_SHAPES)
def test_sum_prefix_every_form(cols, prefix, kind):
    """exact / padded: ``a`` has a row stride of exactly ``prefix``.  padded / wider at cols % 4 != 0: the float4 form's last
    group of a row must leave out[r, cols .. padded) alone, as the header says.  wider: out is a column view of a wider
    NaN buffer.  odd: the scalar form."""
    for rows in PREFIX_ROWS:
        case = prefix_case(rows, cols, prefix)
        for used in SUBSETS:
            if rows == 300 and cols > 1000 and used not in ((1, 1, 1), (0, 0, 0), (0, 1, 0), (1, 0, 1)):
                continue
            run_prefix("sum_prefix %s (%d, %d) %s" % (kind, cols, prefix, "".join(map(str, used))), rows, cols, prefix, kind,
                       used, case)


@pytest.mark.parametrize("cols,prefix", [(8, 4), (40, 24)])
def test_sum_prefix_scalar_form_on_a_misaligned_view(cols, prefix):
    run_prefix("sum_prefix offset view (%d, %d)" % (cols, prefix), 5, cols, prefix, "padded", (1, 1, 1), offset=1)


def test_sum_prefix_past_the_grid_cap():
    rows, cols, prefix = 2500, 1677, 1664
    assert rows * ((cols + 3) // 4) > K_CUS * 16 * 256
    run_prefix("sum_prefix<T> past the grid cap", rows, cols, prefix, "padded", (1, 1, 1))


def test_sum_prefix_refusals():
    base, a, b = prefix_case(5, 8, 4)
    pb, pa, pc, out = Placed(5, 8, base), Placed(5, 4, a), Placed(5, 4, b), Placed(5, 8)

    def call(bs=8, as_=4, cs=4, rows=5, cols=8, prefix=4, os_=8):
        return lib().rbx_sum_prefix(pb.ptr, bs, pa.ptr, as_, pc.ptr, cs, rows, cols, prefix, out.ptr, os_, stream())

    assert call(os_=7) == INVALID and call(bs=7) == INVALID and call(as_=3) == INVALID and call(cs=3) == INVALID
    assert call(prefix=9) == INVALID and call(prefix=-1) == INVALID and call(rows=-1) == INVALID
    assert lib().rbx_sum_prefix(pb.ptr, 8, None, 0, None, 0, 5, 8, 4, None, 8, stream()) == INVALID
    assert call(rows=0) == OK and call(cols=0, prefix=0) == OK
    torch.cuda.synchronize()
    assert out.all_nan()


# ---- scale_by_scalar ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SCALAR_NS + [K_CUS * 8 * 256 + 37])
def test_scale_by_scalar(n):
    x = randn((n,), n)
    sc = torch.tensor([0.37])
    px, ps, out = place(x), place(sc), Placed(1, n)
    assert lib().rbx_scale_by_scalar(px.ptr, ps.ptr, n, out.ptr, stream()) == OK
    assert lib().rbx_scale_by_scalar(px.ptr, ps.ptr, 0, None, stream()) == OK
    torch.cuda.synchronize()
    exact("scale_by_scalar n %d" % n, out.view, G.scale_by_scalar(x, sc)[0])
    assert out.untouched()


@pytest.mark.parametrize("n", [257, 5000])
def test_sigmoid_bce_backward_with_an_upstream_gradient(n):
    """(loss * 0.37).backward(): the upstream scalar is not the unit tensor, so dL/dlogit goes through rbx_scale_by_scalar;
    it must be the float32 product of 0.37 and the gradient that ops.backward(loss) hands back as the forward wrote it."""
    from recbox_amd import ops
    x = (randn((n, 1), n) * 3).cuda()
    y = (randn((n, 1), n + 1) > 0.5).float().cuda()
    x1 = x.clone().requires_grad_(True)
    ops.backward(ops.binary_cross_entropy(ops.sigmoid_output(x1), y))
    x2 = x.clone().requires_grad_(True)
    (ops.binary_cross_entropy(ops.sigmoid_output(x2), y) * 0.37).backward()
    torch.cuda.synchronize()
    assert int(x1.grad.count_nonzero()) > n // 2
    exact("sigmoid_bce dx times 0.37", x2.grad, G.scale_by_scalar(x1.grad, torch.tensor(0.37))[0])


# ---- CIN ------------------------------------------------------------------------------------------------------------------
def run_cin(label, B, F, D, M, kind="randn", seed=0):
    x0, xk, dz = cin_case(B, F, D, M, seed=seed, kind=kind)
    own = xk is None
    m = F if own else M
    p0, pk, pz = place(x0), place(xk), place(dz)
    z = Placed(1, B * D * F * m)
    assert lib().rbx_cin_outer_fwd(p0.ptr, p_(pk), B, F, m, D, z.ptr, stream()) == OK
    torch.cuda.synchronize()
    exact(label + " z", z.view, G.cin_fwd(x0, xk)[0])
    assert z.untouched()
    (wd0, a0), dk = G.cin_bwd(x0, xk, dz)
    for skip in (None, "dx0", "dxk"):
        if own and skip == "dxk":
            continue
        d0, dxk = Placed(1, B * F * D), Placed(1, B * D * m)
        rc = lib().rbx_cin_outer_bwd(p0.ptr, p_(pk), pz.ptr, B, F, m, D, None if skip == "dx0" else d0.ptr,
                                     None if (skip == "dxk" or own) else dxk.ptr, stream())
        assert rc == OK
        torch.cuda.synchronize()
        tag = label + (" without " + skip if skip else "")
        if skip == "dx0":
            assert d0.all_nan()
        else:
            check(tag + " dx0", d0.view, wd0, a0, G.c_cin_dx0(F, m, own))
        if own or skip == "dxk":
            assert dxk.all_nan()
        else:
            check(tag + " dxk", dxk.view, dk[0], dk[1], G.c_cin_dxk(F))
        assert d0.untouched() and dxk.untouched()


@pytest.mark.parametrize("kind", ["randn", "one_signed"])
@pytest.mark.parametrize("B,F,D,M", CIN_SHAPES)
def test_cin_every_shape(B, F, D, M, kind):
    """(2, 39, 40, 200): the backward above 64 KB of LDS, the forward below; (2, 39, 64, 256): both above;
    (2, 130, 8, 130): F + M > 256, the second trip of the backward's t loop; then a small case in the same process."""
    run_cin("cin (%d, %d, %d, %s)" % (B, F, D, M), B, F, D, M, kind)
    if F * D > 1000:
        run_cin("cin (3, 5, 10, 7) after (%d, %d, %d, %s)" % (B, F, D, M), 3, 5, 10, 7, kind, seed=1)


def test_cin_empty_batch_and_refusals():
    """Every refusal is made by cin_check / the NULL tests ahead of any launch."""
    from recbox_amd import ops
    assert lib().rbx_cin_outer_fwd(None, None, 0, 5, 5, 8, None, stream()) == OK
    assert lib().rbx_cin_outer_bwd(None, None, None, 0, 5, 5, 8, None, None, stream()) == OK
    z = ops.cin_outer(torch.zeros(0, 5, 8, device="cuda"))
    assert z.shape == (0, 25)
    x0, xk, dz = cin_case(2, 5, 8, 7)
    p0, pk, pz, z, d0 = place(x0), place(xk), place(dz), Placed(16, 35), Placed(2, 40)
    assert lib().rbx_cin_outer_fwd(p0.ptr, None, 2, 5, 7, 8, z.ptr, stream()) == INVALID          # X_k = X_0 needs M == F
    assert lib().rbx_cin_outer_bwd(p0.ptr, None, pz.ptr, 2, 5, 7, 8, d0.ptr, None, stream()) == INVALID
    assert lib().rbx_cin_outer_fwd(p0.ptr, pk.ptr, 2, 5, 7, 0, z.ptr, stream()) == INVALID
    assert lib().rbx_cin_outer_fwd(p0.ptr, pk.ptr, 2, 5, 7, 8, None, stream()) == INVALID
    # the smallest shapes beyond 160 KB: forward (F + M) D > 40 960 floats, backward (2 F + M) D + F M > 40 960
    big = torch.zeros(20481 * 2, device="cuda")
    bp = ctypes.c_void_p(big.data_ptr())
    assert lib().rbx_cin_outer_fwd(bp, bp, 1, 1, 1, 20481, z.ptr, stream()) == UNSUPPORTED
    assert lib().rbx_cin_outer_bwd(bp, bp, bp, 1, 1, 1, 13654, d0.ptr, None, stream()) == UNSUPPORTED
    torch.cuda.synchronize()
    assert z.all_nan() and d0.all_nan()
    with pytest.raises(NotImplementedError):
        ops.cin_outer(big[:20481].view(1, 1, 20481), big[:20481].view(20481, 1))
    with pytest.raises(ValueError):
        lib_check(lib().rbx_cin_outer_fwd(p0.ptr, None, 2, 5, 7, 8, z.ptr, stream()))


def lib_check(rc):
    from recbox_amd._lib import check as the_check
    the_check(rc)


def test_ops_cin_outer_above_64_kb_then_small():
    """Through ops.cin_outer with autograd: xDeepFM's 200 channels at D = 40, then a small layer in the same process."""
    from recbox_amd import ops
    for B, F, D, M in ((2, 39, 40, 200), (3, 5, 10, None)):
        x0, xk, dz = cin_case(B, F, D, M, seed=2)
        a = x0.cuda().requires_grad_(True)
        k = None if xk is None else xk.cuda().requires_grad_(True)
        z = ops.cin_outer(a, k)
        z.backward(dz.cuda())
        torch.cuda.synchronize()
        exact("ops.cin_outer (%d, %d, %d, %s) z" % (B, F, D, M), z, G.cin_fwd(x0, xk)[0])
        (wd0, a0), dk = G.cin_bwd(x0, xk, dz)
        check("ops.cin_outer (%d, %d, %d, %s) dx0" % (B, F, D, M), a.grad, wd0, a0, G.c_cin_dx0(F, M or F, xk is None))
        if k is not None:
            check("ops.cin_outer (%d, %d, %d, %s) dxk" % (B, F, D, M), k.grad, dk[0], dk[1], G.c_cin_dxk(F))


# ---- split_last -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("views", [False, True])
@pytest.mark.parametrize("shape,n", [((2, 8), 3), ((5, 37), 36), ((1, 8), 4), ((2, 3, 8), 3)])
def test_split_last_values_and_both_backward_paths(shape, n, views):
    """Against plain slicing in float64, values equal.  gb as the trailing-column view of a [rows, cols] buffer of its own
    takes _block_behind's shortcut (2-D, rows >= 2: (1, 8) and the 3-D shape concatenate); the same-shaped view of a larger
    storage does not."""
    from recbox_amd import ops
    cols = shape[-1]
    x = randn(shape, 3 + n)
    ga, gb = randn(shape[:-1] + (n,), 5), randn(shape[:-1] + (cols - n,), 6)

    def on_device(how):
        if how == "own buffer":
            buf = torch.zeros(shape, device="cuda")
            buf[..., n:] = gb.cuda()
            return buf[..., n:]
        if how == "larger storage":
            buf = torch.zeros((shape[0] + 1,) + shape[1:], device="cuda")
            buf[:shape[0], ..., n:] = gb.cuda()
            return buf[:shape[0], ..., n:]
        return gb.cuda()

    for how in ("both", "ga None", "gb None", "own buffer", "larger storage"):
        xr = x.double().requires_grad_(True)
        outs_r = [xr[..., :n], xr[..., n:]]
        xc = x.cuda().requires_grad_(True)
        outs_c = list(ops.split_last(xc, n, views=views))
        for oc, orr in zip(outs_c, outs_r):
            assert oc.shape == orr.shape and (views or oc.is_contiguous())
            exact("split_last %s values" % (shape,), oc, orr.detach())
        grads_r = [None if how == "ga None" else ga.double(), None if how == "gb None" else gb.double()]
        grads_c = [None if how == "ga None" else ga.cuda(), None if how == "gb None" else on_device(how)]
        if how in ("own buffer", "larger storage"):
            hit = ops._block_behind(grads_c[1], shape, n) is not None
            assert hit == (how == "own buffer" and len(shape) == 2 and shape[0] >= 2)
        keep = [i for i in range(2) if grads_r[i] is not None]
        torch.autograd.backward([outs_r[i] for i in keep], [grads_r[i] for i in keep])
        torch.autograd.backward([outs_c[i] for i in keep], [grads_c[i] for i in keep])
        torch.cuda.synchronize()
        exact("split_last %s dx, %s" % (shape, how), xc.grad, xr.grad)
