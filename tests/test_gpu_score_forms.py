"""Candidate scoring (rbx_gatherdot_*, rbx_cosdot_*) and the loss epilogues (rbx_softmax_ce_*, rbx_pair_logsigmoid_*,
rbx_bce_mean_*, rbx_sigmoid_bce_mean and its one-pass form) against the float64 restatements of oracle/score64.py at every
form they dispatch, element by element: |got - want| <= C eps32 A + tiny, the constants of that file's docstring.  Every
comparison goes through ``check``; outputs of direct C-ABI calls start NaN-filled, so an unwritten element fails.

gather_dot: units = D / 4 when D % 4 == 0, the tables and x are 16-byte aligned and x_stride % 4 == 0 (the dx kernel looks
at dx and dx_stride instead of x), else D; gatherdot_{fwd,dx}_kernel<G, NV, VEC>, U candidate rows in flight:
  D (float4)        form             U     D (scalar)   form
  4                 <1, 1, true>     4     1            <1, 1, false>     U = 4 throughout
  8                 <2, 1, true>     4     2            <2, 1, false>
  12, 16            <4, 1, true>     4     3            <4, 1, false>
  20, 32            <8, 1, true>     4     7            <8, 1, false>
  36, 64            <16, 1, true>    4     10           <16, 1, false>
  68, 100, 128      <32, 1, true>    4     17           <32, 1, false>
  132, 256          <64, 1, true>    4     33, 63       <64, 1, false>
  260, 512          <64, 2, true>    2     65, 127      <64, 2, false>
  516, 1000, 1024   <64, 4, true>    2     129, 255     <64, 4, false>
  1028              refused                257          refused (RBX_ERR_UNSUPPORTED)
  A float4 dim whose x is misaligned or has x_stride % 4 != 0 runs the scalar form of the same D: <4, 1, false> at 4,
  <16, 1, false> at 16, <64, 1, false> at 64, <64, 4, false> at 132 and 256; at 260 no scalar form exists and
  ops.gather_dot raises NotImplementedError("gatherdot: dim 260 too large") -- it neither copies nor computes.
  The table backward is DotPolicy's instantiation of the sorted reduce (tests/test_gpu_embed_dims.py has its table).
cos_dot: q = D / 4; cosdot_{fwd,bwd}_vec_kernel<G, NV> when D % 4 == 0, q a power of two in 2 .. 64 (G = q, NV = 1) or a
  multiple of 64 up to 256 (G = 64, NV = q / 64), every pointer 16-byte aligned and the outer strides % 4 == 0; else
  cosdot_{fwd,bwd}_kernel<G>, G = min(64, next power of two >= D):
  D      8      16     64      256     512     768     1024    | 4     12     24     6     20     1000
  form   v<2,1> v<4,1> v<16,1> v<64,1> v<64,2> v<64,3> v<64,4> | s<4>  s<16>  s<32>  s<8>  s<32>  s<64>
softmax_ce: a thread per row, 256 rows per workgroup, loss_final_kernel over the block partials (a second trip of its
  loop from 257 partials: rows = 65 536 + 257).  pair_logsigmoid, bce, sigmoid_bce: 1024 elements per workgroup, the same
  final sum (n = 262 144 + 1029: 258 partials).

Worst err / bound observed on the MI355X (the ledger of conftest._note has every label):
  op (cases)                 worst over every form and input
  gather_dot (103)           logits 0.021   dx 0.024   dW 0.030 (accumulate / store 0.016)   per form: all within 0.003 .. 0.030
  cos_dot (72)               out 0.033      du 0.036   dv 0.068 (scalar <4>; the vector forms 0.049 at most)
  softmax_ce (20)            loss 0.011     lse 0.0092 dlogits 0.020     258 partials: loss 0.0030
  pair_logsigmoid (7)        loss 0.0096    dpos 0.019 dneg 0.027
  bce (4)                    loss 0.013     dp 0.023
  sigmoid_bce (5)            prob 0.017     loss 0.031 and dx 0.125 with the conditioning term in the bound;
                             on the device's own prob, without it: loss 0.017, dx 0.013
  211 cases, 5 s for the file (the slowest case 1.1 s, the first to touch the device).  Nothing is above 0.5.
The transcendental allowance T = 6 of every loss bound is 4 x 1.29, the worst float32-on-the-CPU figure
(tests/test_score64_restatement.py::test_float32_formulas_and_the_allowance; per op in oracle/score64.py).

Mutation check (scratch builds, not committed): two single-line faults, each linked into a library of its own.
  (a) DotFrag::load skips its last unit when NV > 1.  tests/test_gpu_matching.py, test_gpu_edge_cases.py and
      test_gpu_embed_dims.py (without its lookup grid) as they were: 214 passed.  This file: 28 failed, exactly the NV > 1
      forms -- every_form at 260, 512, 1000, 1024, 65, 127, 255, candidate_counts at 512 and 65, the scalar form forced at
      256 (not at 132, whose last unit lies beyond the row), the 260 cases and the bad ids at 512.
  (b) loss_final_kernel stops at 256 partials.  Of the same earlier tests one notices:
      test_pair_logsigmoid_epilogue_vs_torch[(4096, 200)] has 800 partials; nothing earlier did for softmax_ce.  This
      file: 4 failed -- softmax_ce_second_trip_of_the_final_sum (both inputs) and the two pair_logsigmoid cases at
      n = 263 173.  (bce and sigmoid_bce have a final kernel of their own, bce_final_kernel, and pass.)"""
import ctypes

import pytest
import torch

from conftest import _note
from oracle import score64 as S
from test_score64_restatement import (BCE_POINTS, BCE_Y, LADDER, SATURATED, bce_case, cos_case, dot_case, pair_case, sce_case,
                                      sigmoid_case)

pytestmark = pytest.mark.gpu

EPS32, TINY = S.EPS32, S.TINY
DOT_VEC = [4, 8, 12, 16, 20, 32, 36, 64, 68, 100, 128, 132, 256, 260, 512, 516, 1000, 1024]
DOT_SCALAR = [1, 2, 3, 7, 10, 17, 33, 63, 65, 127, 129, 255]
COS_DIMS = [4, 8, 12, 16, 24, 64, 256, 512, 768, 1024, 6, 20, 1000]
NAN = float("nan")


def check(label, got, want, A, C, extra=None):
    """THE comparison: every element within C eps32 A + tiny (+ extra); notes the worst err / bound under ``label``."""
    got = got.detach().double().cpu().reshape(want.shape)
    assert not bool(torch.isnan(got).any()), "%s: %d elements were never written" % (label, int(torch.isnan(got).sum()))
    bound = C * EPS32 * A + TINY
    if extra is not None:
        bound = bound + extra
    err = (got - want).abs()
    r = float((err / bound).max()) if err.numel() else 0.0
    _note("%s (err / bound)" % label, r, 1.0)
    print("%s: %.3g" % (label, r))
    assert bool((err <= bound).all()), "%s: %.3g x the bound (%d of %d elements)" % (label, r, int((err > bound).sum()), err.numel())


def dot_form(D, vec=None):
    vec = (D % 4 == 0) if vec is None else vec
    units = D // 4 if vec else D
    g = S.lane_group(units)
    return "gather_dot <%d,%d,%s>" % (g, 1 if units <= 64 else (2 if units <= 128 else 4), "T" if vec else "F")


def nan_like(shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device="cuda")


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- gather_dot through ops ---------------------------------------------------------------------------------------------
def run_dot(x_dev, tables, sets, gout, scale, pad=None, train_tables=True, retain=False):
    from recbox_amd import ops
    uniq = []
    for t in tables:
        if not any(t is u for u in uniq):
            uniq.append(t)
    tc = [u.cuda().requires_grad_(train_tables) for u in uniq]
    wl = [tc[[t is u for u in uniq].index(True)] for t in tables]
    xc = x_dev.detach().requires_grad_(True)
    out = ops.gather_dot(xc, [i.cuda() for i in sets], wl, scale=scale, padding_idx=pad)
    out.backward(gout.cuda(), retain_graph=retain)
    torch.cuda.synchronize()
    return out, xc, tc


def check_dot(label, case, out, dx, dws, scale, pad=None):
    x, tables, sets, gout = case
    n_out = gout.shape[1]
    want, A = S.gather_dot(x, tables, sets, scale, pad)
    check(label + " logits", out, want, A, S.c_dot_fwd(x.shape[1]))
    (wdx, a_dx), grads = S.gather_dot_grad(x, tables, sets, gout, scale, pad)
    if dx is not None:
        check(label + " dx", dx, wdx, a_dx, S.c_dot_dx(n_out))
    if dws is not None:
        assert len(dws) == len(grads)
        for got, (w, a) in zip(dws, grads):
            check(label + " dW", got, w, a, S.C_BOUND)


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("D", DOT_VEC + DOT_SCALAR)
def test_gather_dot_every_form(D, shared):
    """Widths 1 (int32 ids) and 2 (int64 ids), n_out = 3: a ragged tail for U = 4 and for U = 2; V = 50, so the sorted
    backward walks long runs of equal ids; over one shared table and over two."""
    case = dot_case(D, shared=shared, kind="one_signed" if shared else "randn")
    out, xc, tc = run_dot(case[0].cuda(), case[1], case[2], case[3], 0.25)
    check_dot(dot_form(D), case, out, xc.grad, [t.grad for t in tc], 0.25)


@pytest.mark.parametrize("widths", [(1,), (1, 3), (2, 3), (1, 2, 3)])
@pytest.mark.parametrize("D", [16, 512, 65])
def test_gather_dot_candidate_counts(D, widths):
    """n_out = 1, 4, 5, 6 against the U-wide candidate loop (U = 4 at 16, 2 at 512 and 65)."""
    case = dot_case(D, widths=widths, seed=3)
    out, xc, tc = run_dot(case[0].cuda(), case[1], case[2], case[3], 1.0)
    check_dot("%s n_out %d" % (dot_form(D), sum(widths)), case, out, xc.grad, [t.grad for t in tc], 1.0)


def misplaced(x, how):
    """x on the device as a view that defeats the float4 form: one float into its storage, or a row stride % 4 != 0."""
    R, D = x.shape
    if how == "offset":
        base = torch.zeros(R * D + 1, device="cuda")
        view = base[1:].view(R, D)
    else:
        base = torch.zeros(R, D + 3, device="cuda")
        view = base[:, :D]
    view.copy_(x.cuda())
    return view


@pytest.mark.parametrize("how", ["offset", "stride"])
@pytest.mark.parametrize("D", [4, 16, 64, 132, 256])
def test_gather_dot_scalar_form_forced_at_a_float4_dim(D, how):
    case = dot_case(D, seed=5)
    xv = misplaced(case[0], how)
    assert xv.data_ptr() % 16 != 0 or xv.stride(0) % 4 != 0
    out, xc, tc = run_dot(xv, case[1], case[2], case[3], 0.25)
    assert xc.data_ptr() == xv.data_ptr() and xc.stride() == xv.stride()
    check_dot("%s forced by %s" % (dot_form(D, False), how), case, out, xc.grad, [t.grad for t in tc], 0.25)


@pytest.mark.parametrize("how", ["offset", "stride"])
def test_gather_dot_at_260_has_no_scalar_form_and_says_so(how):
    """ops.gather_dot hands a unit-inner-stride x to the kernel as it is; beyond 256 floats no scalar form exists and the
    C ABI refuses: the documented NotImplementedError, never a silently wrong result."""
    case = dot_case(260, seed=5)
    xv = misplaced(case[0], how)
    with pytest.raises(NotImplementedError, match="gatherdot: dim 260 too large"):
        run_dot(xv, case[1], case[2], case[3], 0.25)
    out, xc, tc = run_dot(xv.clone(), case[1], case[2], case[3], 0.25)       # the same values, aligned: computed
    check_dot(dot_form(260) + " after the refusal", case, out, xc.grad, [t.grad for t in tc], 0.25)


@pytest.mark.parametrize("D,groups", [(256, 4), (16, 64)])
def test_gather_dot_past_the_grid_cap(D, groups):
    """The forward and dx launch at most kCUs * 16 = 4096 workgroups of 256 / G lane groups: rows = cap * groups + 37 gives
    the grid-stride loop a second, ragged trip."""
    R = 4096 * groups + 37
    case = dot_case(D, R=R, seed=7)
    out, xc, _ = run_dot(case[0].cuda(), case[1], case[2], case[3], 0.5, train_tables=False)
    check_dot("%s past the grid cap" % dot_form(D), case, out, xc.grad, None, 0.5)


def test_gather_dot_padding_row_is_scored_and_gets_no_gradient():
    case = dot_case(20, seed=9, shared=True)
    pad = 7
    assert bool((case[2][0] == pad).any()) and bool((case[2][1] == pad).any())
    out, xc, tc = run_dot(case[0].cuda(), case[1], case[2], case[3], 1.0, pad=pad)
    check_dot(dot_form(20) + " padding row", case, out, xc.grad, [t.grad for t in tc], 1.0, pad=pad)
    assert int(tc[0].grad[pad].count_nonzero()) == 0
    assert bool((out[(case[2][0] == pad).cuda(), 0] != 0).all())


@pytest.mark.parametrize("D", [16, 260, 65])
def test_gather_dot_same_bits_on_repeat(D):
    case = dot_case(D, seed=11)
    out, xc, tc = run_dot(case[0].cuda(), case[1], case[2], case[3], 0.25, retain=True)
    first = [out.detach().clone(), xc.grad.clone()] + [t.grad.clone() for t in tc]
    xc.grad = None
    for t in tc:
        t.grad = None
    out.backward(case[3].cuda())                      # backward twice over one forward
    torch.cuda.synchronize()
    for a, b in zip(first[1:], [xc.grad] + [t.grad for t in tc]):
        assert torch.equal(a, b)
    out2, xc2, tc2 = run_dot(case[0].cuda(), case[1], case[2], case[3], 0.25)     # two calls on the same inputs
    for a, b in zip(first, [out2.detach(), xc2.grad] + [t.grad for t in tc2]):
        assert torch.equal(a, b)


# ---- gather_dot on the C ABI --------------------------------------------------------------------------------------------
class DotAbi(object):
    """A case bound to rbx_field_t descriptors: every id set [R, n] over its table, gradients in ``grads``."""

    def __init__(self, case, pad=None, grads=None):
        from recbox_amd import ops
        from recbox_amd._lib import FIELD_CATEGORICAL, POOL_CONCAT
        self.x, tables, sets, self.gout = case
        self.R, self.D = self.x.shape
        self.uniq = []
        for t in tables:
            if not any(t is u for u in self.uniq):
                self.uniq.append(t)
        index = [[t is u for u in self.uniq].index(True) for t in tables]
        specs, col = [], 0
        self.ids = [i.reshape(self.R, -1).cuda() for i in sets]
        for s, (ids, pi) in enumerate(zip(self.ids, index)):
            specs.append(ops.FieldSpec("set%d" % s, FIELD_CATEGORICAL, self.D, col, param=pi, pool=POOL_CONCAT,
                                       seq_len=ids.shape[1], vocab=self.uniq[pi].shape[0], padding_idx=pad))
            col += ids.shape[1]
        self.n_out = col
        self.plan = ops.EmbedPlan(specs, col)
        self.tc = [u.cuda().contiguous() for u in self.uniq]
        self.grads = grads if grads is not None else [torch.zeros_like(t) for t in self.tc]
        self.plan.bind_inputs(self.ids)
        self.plan.bind_params(self.tc, self.grads)
        self.xc, self.gc = self.x.cuda().contiguous(), self.gout.cuda().contiguous()

    def forward(self, scale):
        from recbox_amd._lib import lib
        out = nan_like((self.R, self.n_out))
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        rc = lib.rbx_gatherdot_fwd(self.plan.arr, self.plan.n, self.R, ptr(self.xc), self.xc.stride(0), scale, ptr(out),
                                   ptr(status), stream())
        torch.cuda.synchronize()
        return rc, out, int(status.item())

    def backward(self, scale, dx, dx_stride, accumulate):
        from recbox_amd._lib import lib
        nbytes = lib.rbx_gatherdot_bwd_workspace_size(self.plan.arr, self.plan.n, self.R)
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device="cuda")
        rc = lib.rbx_gatherdot_sort(self.plan.arr, self.plan.n, self.R, ptr(ws), nbytes, None, stream())
        if rc != 0:
            return rc
        rc = lib.rbx_gatherdot_bwd(self.plan.arr, self.plan.n, self.R, ptr(self.xc), self.xc.stride(0), ptr(self.gc), scale,
                                   ptr(dx), dx_stride, accumulate, ptr(ws), nbytes, stream())
        torch.cuda.synchronize()
        return rc


@pytest.mark.parametrize("extra", [4, 3])
@pytest.mark.parametrize("D", [16, 260])
def test_gatherdot_bwd_writes_dx_inside_a_wider_row_and_nothing_else(D, extra):
    """dx_stride = D + 4 keeps the float4 store, D + 3 selects the scalar dx kernel; the columns outside [0, D) stay NaN."""
    abi = DotAbi(dot_case(D, R=67, seed=13))
    if D == 260 and extra == 3:
        buf = nan_like((abi.R, D + extra))
        assert abi.backward(0.5, buf, D + extra, 0) == -4          # RBX_ERR_UNSUPPORTED: no scalar dx form beyond 256
        assert bool(torch.isnan(buf).all())
        return
    buf = nan_like((abi.R, D + extra))
    assert abi.backward(0.5, buf, D + extra, 0) == 0
    assert bool(torch.isnan(buf[:, D:]).all())
    case = (abi.x, [abi.uniq[0], abi.uniq[1]], [i.cpu() for i in abi.ids], abi.gout)
    (wdx, a_dx), grads = S.gather_dot_grad(*case, 0.5)
    check("%s dx in a wider row" % dot_form(D, extra == 4), buf[:, :D], wdx, a_dx, S.c_dot_dx(abi.n_out))
    for got, (w, a) in zip(abi.grads, grads):
        check("%s dW (C ABI)" % dot_form(D), got, w, a, S.C_BOUND)


@pytest.mark.parametrize("accumulate", [1, 0])
@pytest.mark.parametrize("D", [12, 129])
def test_gatherdot_bwd_accumulate_contract(D, accumulate):
    """accumulate = 1: old gradient + the batch's, rows the batch did not name bit-identical.  accumulate = 0 (the header:
    "the caller pre-zeroed the grads, touched rows are stored (no read)"): named rows hold the batch's gradient alone,
    whatever they held; the others keep what they held."""
    case = dot_case(D, R=19, seed=15)
    g = torch.Generator().manual_seed(D)
    old = [torch.randn(50, D, generator=g) for _ in range(2)]
    abi = DotAbi(case, grads=[o.cuda().clone() for o in old])
    assert abi.backward(2.0, None, D, accumulate) == 0
    _, grads = S.gather_dot_grad(*case, 2.0)
    for got, o, (w, a) in zip(abi.grads, old, grads):
        named = (a.sum(1) > 0)
        assert 0 < int(named.sum()) < 50
        assert torch.equal(got.cpu()[~named], o[~named])
        if accumulate:
            check("%s dW accumulate" % dot_form(D), got.cpu()[named], (o.double() + w)[named], (o.double().abs() + a)[named], S.C_BOUND)
        else:
            check("%s dW store" % dot_form(D), got.cpu()[named], w[named], a[named], S.C_BOUND)


@pytest.mark.parametrize("D", [16, 7, 512])
def test_gatherdot_out_of_range_ids_raise_the_status_and_score_zero(D):
    x, tables, sets, gout = dot_case(D, R=67, seed=17)
    sets = [sets[0].clone().reshape(-1, 1), sets[1].clone()]
    sets[0][3, 0] = 50                              # == vocab
    sets[1][9, 1] = -1
    case = (x, tables, sets, gout)
    abi = DotAbi(case)
    rc, out, status = abi.forward(0.5)
    assert rc == 0 and (status & 1) == 1
    assert float(out[3, 0]) == 0.0 and float(out[9, 2]) == 0.0
    dx = nan_like((abi.R, D))
    assert abi.backward(0.5, dx, D, 0) == 0
    check_dot(dot_form(D) + " bad ids", case, out, dx, abi.grads, 0.5)
    clean = DotAbi(dot_case(D, R=67, seed=17))
    assert clean.forward(0.5)[2] == 0


@pytest.mark.parametrize("D", [1028, 257])
def test_gatherdot_refuses_dims_beyond_its_forms(D):
    abi = DotAbi(dot_case(D, R=5, seed=19))
    rc, out, _ = abi.forward(1.0)
    assert rc == -4 and bool(torch.isnan(out).all())                      # RBX_ERR_UNSUPPORTED, nothing written
    dx = nan_like((abi.R, D))
    for g in abi.grads:
        g.fill_(NAN)
    assert abi.backward(1.0, dx, D, 0) == -4
    assert bool(torch.isnan(dx).all()) and all(bool(torch.isnan(g).all()) for g in abi.grads)


# ---- cos_dot --------------------------------------------------------------------------------------------------------------
def cos_form(D, vec_ok=True):
    q = D // 4
    if vec_ok and D % 4 == 0 and ((2 <= q <= 64 and q & (q - 1) == 0) or (q % 64 == 0 and q // 64 <= 4)):
        return "cos_dot vec <%d,%d>" % (min(q, 64), max(1, q // 64))
    return "cos_dot scalar <%d>" % S.lane_group(D)


def check_cos(label, case, D, N, out, du, dv, scale):
    u, v, g = case
    want, A = S.cos_dot(u, v, 1e-12, scale)
    check(label + " out", out, want, A, S.c_cos_fwd(D))
    assert float(out.detach()[1, 0]) == 0.0          # the zero candidate row
    (wdu, a_du), (wdv, a_dv) = S.cos_dot_grad(u, v, g, 1e-12, scale)
    if du is not None:
        check(label + " du", du, wdu, a_du, S.c_cos_du(D, N))
    if dv is not None:
        check(label + " dv", dv, wdv, a_dv, S.c_cos_dv(D))


@pytest.mark.parametrize("kind", ["randn", "one_signed"])
@pytest.mark.parametrize("N", [1, 5])
@pytest.mark.parametrize("D", COS_DIMS)
def test_cos_dot_every_form(D, N, kind):
    from recbox_amd import ops
    case = cos_case(D, N, B=257, kind=kind)
    u, v = case[0].cuda().requires_grad_(True), case[1].cuda().requires_grad_(True)
    out = ops.cos_dot(u, v, eps=1e-12, scale=20.0)
    out.backward(case[2].cuda())
    torch.cuda.synchronize()
    check_cos(cos_form(D), case, D, N, out, u.grad, v.grad, 20.0)
    u2, v2 = case[0].cuda().requires_grad_(True), case[1].cuda().requires_grad_(True)
    out2 = ops.cos_dot(u2, v2, eps=1e-12, scale=20.0)
    out2.backward(case[2].cuda())
    assert torch.equal(out, out2) and torch.equal(u.grad, u2.grad) and torch.equal(v.grad, v2.grad)


def block_view(v, lead, tail, fill=0.0):
    """v [B, N, D] as a view behind ``lead`` columns of a [B, lead + N D + tail] block on the device."""
    B, N, D = v.shape
    base = torch.full((B, lead + N * D + tail), fill, device="cuda")
    view = base[:, lead:lead + N * D].view(B, N, D)
    return base, view


@pytest.mark.parametrize("lead,tail", [(8, 4), (8, 5)])
@pytest.mark.parametrize("D", [8, 64, 768, 12])
def test_cos_dot_reads_v_in_place_inside_a_wider_row(D, lead, tail):
    """outer stride % 4 == 0 keeps the vector kernels (where D has one); % 4 != 0 must select the scalar ones."""
    from recbox_amd import ops
    N = 5
    case = cos_case(D, N, B=67, seed=3)
    _, view = block_view(case[1], lead, tail)
    view.copy_(case[1].cuda())
    u, v = case[0].cuda().requires_grad_(True), view.detach().requires_grad_(True)
    assert v.stride() == (lead + N * D + tail, D, 1) and v.data_ptr() == view.data_ptr()
    out = ops.cos_dot(u, v, eps=1e-12, scale=20.0)
    out.backward(case[2].cuda())
    torch.cuda.synchronize()
    check_cos("%s in a wider row" % cos_form(D, (lead + N * D + tail) % 4 == 0), case, D, N, out, u.grad, v.grad, 20.0)


def cos_abi(case, D, N, v_dev, v_outer, du, dv, dv_outer, scale=20.0):
    from recbox_amd._lib import lib
    B = case[0].shape[0]
    u, g = case[0].cuda().contiguous(), case[2].cuda().contiguous()
    out, inv = nan_like((B, N)), nan_like((B, N))
    assert lib.rbx_cosdot_fwd(ptr(u), ptr(v_dev), v_outer, B, N, D, 1e-12, scale, ptr(out), ptr(inv), stream()) == 0
    assert lib.rbx_cosdot_bwd(ptr(u), ptr(v_dev), v_outer, ptr(inv), ptr(g), B, N, D, scale, ptr(du), ptr(dv), dv_outer,
                              stream()) == 0
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("lead,tail", [(4, 4), (4, 3), (1, 3)])
@pytest.mark.parametrize("D", [16, 768, 24])
def test_cosdot_bwd_writes_dv_inside_a_wider_row_and_nothing_else(D, lead, tail):
    """dv into a NaN-filled block (stride % 4 == 0 and aligned; stride % 4 != 0; misaligned): the columns outside stay NaN."""
    N = 5
    case = cos_case(D, N, B=67, seed=5)
    v = case[1].cuda().contiguous()
    base, dv = block_view(case[1], lead, tail, fill=NAN)
    du = nan_like((67, D))
    out = cos_abi(case, D, N, v, N * D, du, dv, base.stride(0))
    vec = base.stride(0) % 4 == 0 and lead % 4 == 0
    check_cos("%s dv in a wider row" % cos_form(D, vec), case, D, N, out, du, dv, 20.0)
    assert bool(torch.isnan(base[:, :lead]).all()) and bool(torch.isnan(base[:, lead + N * D:]).all())


@pytest.mark.parametrize("D", [16, 768, 24])
def test_cosdot_bwd_null_outputs(D):
    N = 5
    case = cos_case(D, N, B=67, seed=7)
    v = case[1].cuda().contiguous()
    du, dv = nan_like((67, D)), nan_like((67, N, D))
    out = cos_abi(case, D, N, v, N * D, du, None, N * D)
    check_cos(cos_form(D) + " d_dv NULL", case, D, N, out, du, None, 20.0)
    out = cos_abi(case, D, N, v, N * D, None, dv, N * D)
    check_cos(cos_form(D) + " d_du NULL", case, D, N, out, None, dv, 20.0)


# ---- softmax cross entropy --------------------------------------------------------------------------------------------------
def sce_abi(x, t, strided=False, g=1.0):
    """(loss, lse, dlogits, status) of rbx_softmax_ce_fwd / _bwd; strided: the logits are the leading columns of [rows, n + 3]."""
    from recbox_amd._lib import lib
    rows, n = x.shape
    if strided:
        base = nan_like((rows, n + 3))
        xd = base[:, :n]
        xd.copy_(x.cuda())
    else:
        xd = x.cuda().contiguous()
    stride = xd.stride(0) if rows > 1 else (n + 3 if strided else n)
    td = t.cuda() if t is not None else None
    loss, lse, dx = nan_like((1,)), nan_like((rows,)), nan_like((rows, n))
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    nbytes = lib.rbx_loss_workspace_size(rows)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    gd = torch.full((1,), g, device="cuda")
    assert lib.rbx_softmax_ce_fwd(ptr(xd), stride, rows, n, ptr(td), ptr(loss), ptr(lse), ptr(status), ptr(ws), nbytes,
                                  stream()) == 0
    assert lib.rbx_softmax_ce_bwd(ptr(xd), stride, rows, n, ptr(td), ptr(lse), ptr(gd), ptr(dx), stream()) == 0
    torch.cuda.synchronize()
    return loss, lse, dx, int(status.item())


def check_sce(label, x, t, got, g=1.0):
    loss, lse, dx, _ = got
    rows, n = x.shape
    (wl, al), (wlse, a_lse) = S.softmax_ce(x, t)
    check(label + " loss", loss, wl.reshape(1), al.reshape(1), S.c_loss(n + 4, -(-rows // 256)))
    check(label + " lse", lse, wlse, a_lse, S.c_loss(n + 4, 1))
    wdx, a_dx = S.softmax_ce_grad(x, t, g)
    check(label + " dlogits", dx, wdx, a_dx, S.c_loss(n + 4, 1))
    gone = torch.isinf(x)
    assert int(dx.cpu()[gone].count_nonzero()) == 0
    if n == 1:
        assert float(loss) == 0.0 and torch.equal(lse.cpu(), x.reshape(-1)) and int(dx.count_nonzero()) == 0


@pytest.mark.parametrize("n", [1, 2, 5, 101])
@pytest.mark.parametrize("rows", [1, 255, 256, 257])
def test_softmax_ce_every_input_and_target(rows, n):
    for kind in ("randn4", "uniform100", "constant", "masked"):
        for target in ("none", "random", "last"):
            x, t = sce_case(kind, rows, n, target=target)
            for strided in (False, True):
                got = sce_abi(x, t, strided, g=1.5)
                assert got[3] == 0
                check_sce("softmax_ce %s" % kind, x, t, got, g=1.5)
    again = sce_abi(x, t, True, g=1.5)
    assert all(torch.equal(a, b) for a, b in zip(got[:3], again[:3]))


@pytest.mark.parametrize("kind", ["randn4", "one_signed"])
def test_softmax_ce_second_trip_of_the_final_sum(kind):
    """rows = 65 536 + 257, n = 2: 258 block partials, thread 0 and 1 of loss_final_kernel add two each."""
    rows = 65536 + 257
    if kind == "randn4":
        x, t = sce_case(kind, rows, 2)
    else:                                           # every row's term about the same and positive: a lost partial shows
        x = torch.rand(rows, 2, generator=torch.Generator().manual_seed(1)) + 0.5
        t = torch.zeros(rows, dtype=torch.long)
    got = sce_abi(x, t)
    check_sce("softmax_ce 258 partials %s" % kind, x, t, got)
    assert all(torch.equal(a, b) for a, b in zip(got[:3], sce_abi(x, t)[:3]))


@pytest.mark.parametrize("bad", [5, -1])
def test_softmax_ce_out_of_range_target_raises_the_status_and_scores_as_target_zero(bad):
    x, t = sce_case("randn4", 257, 5)
    t2 = t.clone()
    t2[100] = bad
    got = sce_abi(x, t2)
    assert (got[3] & 1) == 1
    t0 = t.clone()
    t0[100] = 0
    check_sce("softmax_ce bad target", x, t0, got)
    assert sce_abi(x, t0)[3] == 0


# ---- pairwise log-sigmoid ---------------------------------------------------------------------------------------------------
def pair_abi(pos, neg, w, scale, g=1.0):
    from recbox_amd._lib import lib
    n = pos.numel()
    pd, nd = pos.cuda().contiguous(), neg.cuda().contiguous()
    wd = w.cuda().contiguous() if w is not None else None
    loss, dp, dn = nan_like((1,)), nan_like((n,)), nan_like((n,))
    nbytes = lib.rbx_loss_workspace_size(n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    gd = torch.full((1,), g, device="cuda")
    assert lib.rbx_pair_logsigmoid_fwd(ptr(pd), ptr(nd), ptr(wd), n, scale, ptr(loss), ptr(ws), nbytes, stream()) == 0
    assert lib.rbx_pair_logsigmoid_bwd(ptr(pd), ptr(nd), ptr(wd), ptr(gd), n, scale, ptr(dp), ptr(dn), stream()) == 0
    torch.cuda.synchronize()
    return loss, dp, dn


def check_pair(label, pos, neg, w, scale, got, g=1.0):
    n = pos.numel()
    (wl, al), _ = S.pair_logsigmoid(pos, neg, w, scale)
    check(label + " loss", got[0], wl.reshape(1), al.reshape(1), S.c_loss(4, -(-n // 1024)))
    (wdp, a_dp), (wdn, a_dn) = S.pair_logsigmoid_grad(pos, neg, w, scale, g)
    check(label + " dpos", got[1], wdp, a_dp, S.c_elem())
    check(label + " dneg", got[2], wdn, a_dn, S.c_elem())


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 262144 + 1029])
def test_pair_logsigmoid_every_input_and_weight(n):
    for kind in ("randn6", "uniform100"):
        for weight in ("none", "mask", "positive"):
            pos, neg, w = pair_case(kind, n, weight=weight)
            scale = 1.0 / n if weight != "mask" else 1.0
            got = pair_abi(pos, neg, w, scale, g=1.5)
            check_pair("pair_logsigmoid %s" % kind, pos, neg, w, scale, got, g=1.5)
    assert all(torch.equal(a, b) for a, b in zip(got, pair_abi(pos, neg, w, scale, g=1.5)))


@pytest.mark.parametrize("n", [1025, 262144 + 1029])
def test_pair_logsigmoid_masked_positions_cost_nothing_whatever_they_hold(n):
    """inf, -inf and NaN under w == 0: the loss is the unmasked positions', dpos and dneg are exactly 0 there
    (rbx_pair_logsigmoid_bwd used to evaluate w (1 - sigmoid(pos)) unconditionally: 0 * NaN)."""
    pos, neg, w = pair_case("randn6", n, seed=3, weight="mask")
    dead = (w == 0).nonzero().reshape(-1)
    assert dead.numel() >= 3
    pos[dead[0::3]], neg[dead[0::3]] = float("inf"), NAN
    neg[dead[1::3]] = float("-inf")
    pos[dead[2::3]] = NAN
    got = pair_abi(pos, neg, w, 1.0)
    check_pair("pair_logsigmoid masked inf / nan", pos, neg, w, 1.0, got)
    assert int(got[1][dead.cuda()].count_nonzero()) == 0 and int(got[2][dead.cuda()].count_nonzero()) == 0


# ---- BCE on probabilities ---------------------------------------------------------------------------------------------------
def bce_abi(p, y, g=1.0):
    from recbox_amd._lib import lib
    n = p.numel()
    pd, yd = p.cuda().contiguous(), y.cuda().contiguous()
    loss, dp = nan_like((1,)), nan_like((n,))
    nbytes = lib.rbx_bce_workspace_size(n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    gd = torch.full((1,), g, device="cuda")
    assert lib.rbx_bce_mean_fwd(ptr(pd), ptr(yd), n, ptr(loss), ptr(ws), nbytes, stream()) == 0
    assert lib.rbx_bce_mean_bwd(ptr(pd), ptr(yd), ptr(gd), n, ptr(dp), stream()) == 0
    torch.cuda.synchronize()
    return loss, dp


@pytest.mark.parametrize("n", [1, 1025, 262144 + 1029])
def test_bce_mean_with_the_clamp_and_the_guard(n):
    p, y = bce_case(n)
    loss, dp = bce_abi(p, y, g=1.5)
    (wl, al), _ = S.bce(p, y)
    check("bce loss", loss, wl.reshape(1), al.reshape(1), S.c_loss(4, -(-n // 1024)))
    wdp, a_dp = S.bce_grad(p, y, 1.5)
    check("bce dp", dp, wdp, a_dp, S.c_elem())
    loss2, dp2 = bce_abi(p, y, g=1.5)
    assert torch.equal(loss, loss2) and torch.equal(dp, dp2)


def test_bce_mean_clamp_and_guard_point_by_point():
    """p in {0, 1, 1e-30, 1 - 2^-24} x y in {0, 1, 0.3}, one element per call: the clamp at -100 and the 1e-12 guard."""
    for pp in BCE_POINTS:
        for yy in BCE_Y:
            p, y = torch.tensor([pp], dtype=torch.float32), torch.tensor([yy], dtype=torch.float32)
            loss, dp = bce_abi(p, y)
            (wl, al), _ = S.bce(p, y)
            wdp, a_dp = S.bce_grad(p, y, 1.0)
            check("bce points loss", loss, wl.reshape(1), al.reshape(1), S.c_elem())
            check("bce points dp", dp, wdp, a_dp, S.c_elem())
            if pp in (0.0, 1.0) and yy in (0.0, 1.0):
                assert float(loss) == float(wl) and float(wl) in (0.0, 100.0)      # the clamp, exactly
                assert float(dp) == float(wdp.float())                              # (p - y) / 1e-12f, one rounding


# ---- sigmoid + BCE ----------------------------------------------------------------------------------------------------------
def sigmoid_abi(x, y, gs, onepass, counter=None, want_prob=True, want_dx=True):
    from recbox_amd._lib import lib
    n = x.numel()
    xd, yd = x.cuda().contiguous(), y.cuda().contiguous()
    loss = nan_like((1,))
    prob = nan_like((n,)) if want_prob else None
    dx = nan_like((n,)) if want_dx else None
    nbytes = lib.rbx_bce_workspace_size(n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    if onepass:
        assert lib.rbx_sigmoid_bce_mean_onepass(ptr(xd), ptr(yd), n, gs, ptr(prob), ptr(loss), ptr(dx), ptr(ws), nbytes,
                                                ptr(counter), stream()) == 0
    else:
        assert lib.rbx_sigmoid_bce_mean(ptr(xd), ptr(yd), n, gs, ptr(prob), ptr(loss), ptr(dx), ptr(ws), nbytes, stream()) == 0
    torch.cuda.synchronize()
    return loss, prob, dx


def check_sigmoid(label, x, y, gs, got):
    loss, prob, dx = got
    n = x.numel()
    o = S.sigmoid_bce(x, y, gs)
    c = S.c_loss(4, -(-n // 1024))
    k = S.T_ALLOW + 2                                # ulps the device's p may sit from float32(sigmoid64): expf, 1 +, 1 /
    check(label + " prob", prob, o["prob"][0], o["prob"][1], S.c_elem())
    check(label + " loss", loss, o["loss"][0].reshape(1), o["loss"][1].reshape(1), c, extra=k * o["loss"][2].reshape(1))
    check(label + " dx", dx, o["dx"][0], o["dx"][1], S.c_elem(), extra=k * o["dx"][2])
    q = S.sigmoid_bce(x, y, gs, p32=prob)             # on the device's own probabilities: no conditioning term at all
    check(label + " loss of its prob", loss, q["loss"][0].reshape(1), q["loss"][1].reshape(1), c)
    check(label + " dx of its prob", dx, q["dx"][0], q["dx"][1], S.c_elem())
    sat = torch.tensor([float(v) in SATURATED for v in x.tolist()])
    if bool(sat.any()):                              # the saturated rungs, exactly
        assert bool((prob.cpu()[sat] == 1.0).all()) and int(dx.cpu()[sat].count_nonzero()) == 0
        assert torch.equal(q["terms"][0][sat], 100.0 * (1.0 - y.double()[sat]))


@pytest.mark.parametrize("n", [1, 1025, 262144 + 1029])
def test_sigmoid_bce_two_launch_and_onepass(n):
    x, y = sigmoid_case(n)
    counter = torch.zeros(64, dtype=torch.int32, device="cuda")
    two = sigmoid_abi(x, y, 2.0, False)
    check_sigmoid("sigmoid_bce", x, y, 2.0, two)
    for _ in range(2):                               # the second call on the same counter: the same bits
        one = sigmoid_abi(x, y, 2.0, True, counter)
        assert int(counter.count_nonzero()) == 0
        assert all(torch.equal(a, b) for a, b in zip(one, two))
    for onepass in (False, True):
        loss, prob, dx = sigmoid_abi(x, y, 2.0, onepass, counter, want_prob=False)
        assert prob is None and torch.equal(loss, two[0]) and torch.equal(dx, two[2])
        loss, prob, dx = sigmoid_abi(x, y, 2.0, onepass, counter, want_dx=False)
        assert dx is None and torch.equal(loss, two[0]) and torch.equal(prob, two[1])
        assert int(counter.count_nonzero()) == 0


@pytest.mark.parametrize("onepass", [False, True])
def test_sigmoid_bce_saturated_rungs_exactly(onepass):
    """Only x in {17, 20, 88, 110}, each with y = 0 and y = 1: p = 1.0f, term = 100 (1 - y), dx = 0, loss = 50 to the bit."""
    x = torch.tensor(SATURATED + SATURATED)
    y = torch.tensor([0.0] * 4 + [1.0] * 4)
    counter = torch.zeros(64, dtype=torch.int32, device="cuda")
    loss, prob, dx = sigmoid_abi(x, y, 2.0, onepass, counter)
    assert float(loss) == 50.0 and bool((prob == 1.0).all()) and int(dx.count_nonzero()) == 0
    assert int(counter.count_nonzero()) == 0
    assert LADDER.index(17.0) >= 0
