"""BatchNorm, LayerNorm (rbx_norm.hip), Dice and the stand-alone PReLU (rbx_act.hip) through ops.batch_norm / layer_norm /
dice / prelu and, where a form is only reachable below them, the C entry points: every element against the float64
restatement of oracle/norm64.py with |got - want| <= C eps32 A + tiny (C per op as derived there, A = 0 means exactly zero).
Inputs: randn, a mean far from zero (x = 1e3 s + s randn, |mean| rstd up to 1e3), constant columns / rows, gamma == 0
columns, and sign-safe inputs for every ReLU / PReLU case, so that no column is left out of any gradient comparison.

Which body a BatchNorm shape runs (``bn_form`` below restates bn_grid and the kernels' loop tests; the tests assert it).
W = 4 when cols % 4 == 0, else 1; blocks = min(ceil(rows cols / W / 256), 4096); unit = cols / gcd(cols, 256 W); a lane
keeps its columns ("fixed") when blocks >= unit (blocks is then rounded down to a multiple of unit), else the generic loop
with a modulo per element runs; the U-unrolled body of the fixed form runs once rows cols / W > (U - 1) blocks 256 (U = 4
in bn_apply_kernel, 2 in bn_bwd_dx_kernel): on a capped grid, and for U = 2 also where rounding down to a multiple of unit
left fewer lanes than elements, as at (1025, 100):
  cols   W  unit   generic up to rows      cols   W  unit   generic up to rows
  1      1  1      -  (always fixed)        100    4  25     245
  3      1  3      1                        256    4  1      -
  37     1  37     249                      400    4  25     61
  64     4  1      -                        1030   1  515    127
  65     1  65     252                      4099   1  4099   always (unit > the cap of 4096 blocks)
  (33000, 97): scalar, 4074 blocks, both unrolled bodies;  (131072, 100): float4, 4075 blocks, both unrolled bodies.
The reduction chains.  Rows per block R = 64 below 32 768 rows, 256 from there on; nb = ceil(rows / R) partials.
bn_stats_final_kernel (16 wavefronts, wavefront z takes partials z, z + 16, ...): its 16-in-flight loop runs for
nb >= 241, its 8-in-flight loop next for what is left when >= 113 + z remain, then one at a time; bn_bwd_final_kernel
(4 wavefronts): 8 in flight for nb >= 29.
  rows           nb (R)      stats final: 16 / 8 / 1 in flight               bwd final: 8 / 1
  2 .. 64        1           - / - / wavefront 0 only                        - / 1
  65             2           - / - / 1 (the second block holds ONE row: n = 1 merges)
  1025           17 (64)     - / - / 2 for wavefront 0                        - / 1 (4, 5 a wavefront)
  7300           115 (64)    - / wavefronts 0 .. 2 / the rest                 3 times / tail
  16000          250 (64)    wavefronts 0 .. 9 / - / the rest                 7 times / tail
  30000          469 (64)    every wavefront, then 8 in flight, every wavefront 14 times / tail
  32767, 32768   512 (64), 128 (256)     2 x 16 / - / -   and   - / 1 x 8 / -
  70001          274 (256)   16, then tail
LayerNorm <G, NV, VEC>: units = dim / 4 (float4, dim % 4 == 0) or dim; G = min(64, pow2 >= units), NV = pow2 / 64 beyond:
  float4 dim: 4 <1,1> 8 <2,1> 12, 16 <4,1> 20, 32 <8,1> 36, 64 <16,1> 68, 128 <32,1> 132, 200, 256 <64,1> 260, 512 <64,2>
              516, 1000, 1024 <64,4>;   scalar dim: 1 <1,1> 2 <2,1> 3 <4,1> 7 <8,1> 10 <16,1> 17 <32,1> 33, 63 <64,1>
              65, 127 <64,2> 129, 255 <64,4>.
launch_ln gives a lane group one row while ceil(rows / (256 / G)) workgroups fit under the cap (4096, or 1024 when the dx
kernel also leaves the parameter-gradient partials): 5000 rows at dims 64 and 7 are 313 and 157 workgroups, one row a group,
and fill several workgroups' partials for the final kernel; only (300000, 16) makes a group walk several rows (5).
Dims 257, 1023 (scalar units > 256) and 1025, 1028 (> 1024) have no form:
rbx_layernorm_fwd returns RBX_ERR_UNSUPPORTED and ops.layer_norm raises NotImplementedError("layernorm: dim ... too large
for one lane group") -- pinned below.  The reference's nn.LayerNorm has no such limit; a model with such a width must keep
torch's module.
ops.batch_norm with one row in training raises ValueError("Expected more than 1 value per channel when training"), as
torch does; the split entry points take one row (a rank's share of a synchronised batch may be one row).
Constant columns come out of BatchNorm as y == beta exactly (a Welford step on a constant has d == 0: the mean is the
constant, M2 zero) and that is asserted.  Constant ROWS do not come out of LayerNorm exactly: its mean is a float32 sum
times 1 / dim, and 3 c or c / 12 is not a float32 in general, so x - mean is a few ulp of c and y - beta that times rstd
(1e4 at eps = 1e-8).  That is arithmetic torch float32 shares, not a defect: such rows are held to the bound, whose A
carries |mean| rstd.

Fixed with this file: bn_bwd_dx chose the float4 form from the alignment of x, dy and dx alone and then read the ReLU mask
y_relu with float4 loads too; a y_relu that is not 16-byte aligned now selects the scalar form (pinned below through the
C ABI, with dx inside a NaN-filled wider buffer).

Worst err / bound achieved on the MI355X (117 cases, 17 s; every op below 0.1 of its bound, so nothing near 0.5; the
session ledger written by conftest holds every figure per test):
  BatchNorm through ops   y 0.083 (affine=False, randn), evaluation 0.032; dx 0.012 / 0.015; dgamma 0.021 / 0.026 (cols 1030,
                          generic loop, far-from-zero mean); dbeta 0.016; dslope 0.013 / 0.017; running mean 0.031, var 0.023
  reduction chains, capped grids   every output below 0.03 (y in evaluation mode 0.028 at (131072, 100))
  statistics (C entry)    mean 0.031 (16000 rows, far-from-zero mean), rstd 0.012, raw M2 0.017; y given the statistics 0.016
  split entry points      mean 0.018, M2 0.012, y 0.013, dx 0.0062, dgamma 0.011, dbeta 0.0076
  misaligned operands     y 0.014, dx 0.0099, dgamma 0.011, dslope 0.0078
  LayerNorm, every form   y 0.099 ((300000, 16)), dx 0.02, dgamma 0.014, dbeta 0.017; row mean 0.031, rstd 0.0061
  Dice                    y 0.013, dx 0.0079, dalpha 0.0076, running mean 0.02, var 0.011
  PReLU                   y and dx equal; dslope per column 0.014, one slope 0.0068
Dice's 1 - p is a float32 subtraction from a rounded p, so its error magnitude is 1 and not 1 - p: in evaluation mode on
far-from-zero inputs (xhat in the thousands, 1 - p below eps32) dalpha's error scales with |dy x|; oracle/norm64.py's
magnitudes carry that term.  Dice and the stand-alone PReLU take the row counts above 1025 at cols 37, 64 and 65 only (a
scalar count below and above one column block and a cols % 4 == 0 one): their kernels have one element-wise form and the
sequential final sums do not depend on cols, so the wide column counts stop at 1025 rows to keep the float64 side short.
Mutation check (three wrong variants of rbx_norm.hip in a scratch build, not kept; of the GPU tests that existed before
this file, the 319 of the files that reach these kernels -- test_gpu_activations, _matching, _ranking, _seqblock,
_edge_cases -- were run, the others launch none of them; this file has 117):
  (a) bn_apply_kernel's generic loop reads gamma[c] for all four lanes of a float4      1 of 319 failed, 15 of 117 here
      (cols 100 and 400 of the rows x cols grid, 9 of the 11 variants, the split entry points at chunks 1 and 65)
  (b) bn_stats_final_kernel's 8-in-flight loop skips its last partial                   7 of 319 failed, 9 of 117 here
      (the reduction chains and the statistics at 7300, 16000, 30000 and 32768 rows, (33000, 97))
  (c) ln_fwd_kernel sums the variance without the index(...) >= 0 guard                 2 of 319 failed, 21 of 117 here
      (every dim that does not fill its lane group: 12, 20, 36, 68, 132, 200, 260, 516, 1000 and all scalar dims from 3 on)
"""
import ctypes
import math

import pytest
import torch
from torch import nn

from oracle import norm64 as N
from test_gpu_interact_dims import Worst
from test_norm64_restatement import (FAMILIES, ROW_FAMILIES, affine, assert_sign_safe, dice_alpha, randn, sign_safe,
                                     slopes)

pytestmark = pytest.mark.gpu

EPS = 1e-5
BIG_ROWS = [7300, 16000, 30000, 32767, 32768, 70001]
SMALL_ROWS = [2, 3, 5, 33, 64, 65, 1025]


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def bn_form(rows, cols, vec=None):
    """(W, "fixed" | "generic", whether the unrolled body of bn_apply_kernel runs, ... of bn_bwd_dx_kernel)."""
    W = 4 if (cols % 4 == 0 if vec is None else vec) else 1
    total = rows * cols // W
    blocks = min((total + 255) // 256, 4096)
    unit = cols // math.gcd(cols, 256 * W)
    if unit <= blocks:
        blocks = blocks // unit * unit
    fixed = (blocks * 256 * W) % cols == 0
    return W, "fixed" if fixed else "generic", fixed and total > 3 * blocks * 256, fixed and total > blocks * 256


def test_the_shapes_reach_the_bodies_the_table_says():
    assert [bn_form(r, 100)[1] for r in (8, 245, 246)] == ["generic", "generic", "fixed"]
    assert [bn_form(r, 37)[1] for r in (33, 249, 250)] == ["generic", "generic", "fixed"]
    assert [bn_form(r, 400)[1] for r in (61, 62)] == ["generic", "fixed"]
    assert [bn_form(r, 1030)[1] for r in (127, 128)] == ["generic", "fixed"]
    assert [bn_form(r, 65)[1] for r in (252, 253)] == ["generic", "fixed"]
    assert all(bn_form(r, c)[1] == "fixed" for r in (2, 70001) for c in (1, 64, 256))
    assert bn_form(33, 4099)[:2] == (1, "generic") and bn_form(70001, 4099)[1] == "generic"
    assert bn_form(33000, 97) == (1, "fixed", True, True) and bn_form(131072, 100) == (4, "fixed", True, True)
    assert bn_form(70001, 100)[2:] == (False, True) and bn_form(1025, 100)[2:] == (False, True) and bn_form(246, 100)[2:] == (False, False)
    assert N.ln_form(257) is None and N.ln_form(1023) is None and N.ln_form(1025) is None and N.ln_form(1028) is None
    assert N.ln_form(1024) == (64, 4, True) and N.ln_form(255) == (64, 4, False) and N.ln_form(127) == (64, 2, False)


# ---- BatchNorm through ops.batch_norm ----------------------------------------------------------------------------------------
def _bn_run(w, label, rows, cols, family, act=None, affine_=True, track=True, momentum=0.1, x_grad=True, steps=2, seed=0,
            eval_=True):
    """Two training steps, then evaluation mode, of ops.batch_norm on an nn.BatchNorm1d (+ ReLU / nn.PReLU)."""
    from recbox_amd import ops
    gamma0 = family == "gamma0"
    gamma, beta = affine(cols, cols + seed, gamma0=gamma0) if affine_ else (None, None)
    make = FAMILIES["far_mean" if gamma0 else family]
    bn = nn.BatchNorm1d(cols, eps=EPS, momentum=momentum, affine=affine_, track_running_stats=track).cuda()
    pre = None
    if act in ("prelu1", "preluC"):
        pre = nn.PReLU(1 if act == "prelu1" else cols).cuda()
        with torch.no_grad():
            pre.weight.copy_(slopes(cols, act == "preluC", 3).cuda())
    slope = pre.weight.detach().cpu() if pre is not None else None
    if affine_:
        with torch.no_grad():
            bn.weight.copy_(gamma.cuda()), bn.bias.copy_(beta.cuda())
    zero, one = torch.zeros(cols, dtype=torch.float64), torch.ones(cols, dtype=torch.float64)
    rm, rv, nbt = (zero, zero), (one, one), 0
    tag0 = "[%d, %d] %s %s W%d %s" % ((rows, cols, family, act) + bn_form(rows, cols)[:2])
    edge = family == "constant" and act is not None      # xhat == 0 in every element: z == beta, beta == 0 in every other column
    if edge:
        beta[::2] = 0.0
        with torch.no_grad():
            bn.bias.copy_(beta.cuda())
    for step in range(steps + (1 if eval_ else 0)):
        training = step < steps
        bn.train(training)
        stat_rows = rows if (training or not track) else None
        if stat_rows is None:
            mean = bn.running_mean.detach().cpu().double()
            rstd = 1.0 / torch.sqrt(bn.running_var.detach().cpu().double() + N.f32(EPS))
        else:
            mean = rstd = None
        x = make((rows, cols), 100 * seed + 10 * step + rows)
        if act is not None and not edge:
            x = sign_safe(x, gamma, beta, EPS, N.c_bn_y(stat_rows), mean, rstd)
            assert_sign_safe(x, gamma, beta, EPS, N.c_bn_y(stat_rows), mean, rstd)
        dy = randn((rows, cols), step + 7)
        xc = x.cuda().requires_grad_(x_grad)
        bn.zero_grad()
        if pre is not None:
            pre.zero_grad()
        y = ops.batch_norm(xc, bn, relu=act == "relu", prelu=pre)
        y.backward(dy.cuda())
        torch.cuda.synchronize()
        tag = "%s step %d" % (tag0, step)
        mode = "" if training else " eval"
        f = N.bn_fwd64(x, gamma, beta, EPS, relu=act == "relu", slope=slope, mean=mean, rstd=rstd)
        w.add(label + " y" + mode, tag, y, *f["y"], N.c_bn_y(stat_rows))
        b = N.bn_bwd64(x, dy, gamma, f["mean"], f["rstd"], stat_rows is not None,
                       relu_mask=(f["y"][0] > 0) if act == "relu" else None, slope=slope, beta=beta)
        if x_grad:
            w.add(label + " dx" + mode, tag, xc.grad, *b["dx"], N.c_bn_dx(rows, stat_rows))
        else:
            assert xc.grad is None
        if affine_:
            w.add(label + " dgamma" + mode, tag, bn.weight.grad, *b["dgamma"], N.c_bn_dgamma(rows, stat_rows))
            w.add(label + " dbeta" + mode, tag, bn.bias.grad, *b["dbeta"], N.c_bn_sum(rows))
        if act == "preluC":
            w.add(label + " dslope" + mode, tag, pre.weight.grad, *b["dslope"], N.c_bn_dgamma(rows, stat_rows))
        elif act == "prelu1":                 # (the wrapper adds the columns with torch.sum: a tree, inside one more floor)
            w.add(label + " dslope" + mode, tag, pre.weight.grad, b["dslope"][0].sum().reshape(1),
                  b["dslope"][1].sum().reshape(1), N.c_bn_dgamma(rows, stat_rows) + N.C_BOUND)
        if family == "constant" and stat_rows is not None:
            want = beta.float().expand(rows, -1) if affine_ else torch.zeros(rows, cols)
            if act == "relu":
                want = want.clamp_min(0.0)
            elif act is not None:                                  # ONE float32 product on the slope side
                want = torch.where(want > 0, want, slope.float().expand(cols) * want)
            assert torch.equal(y.detach().cpu(), want), tag + ": y != act(beta) on constant columns"
            if edge:
                assert int(torch.count_nonzero(bn.weight.grad)) == 0, tag + ": dgamma != 0 with xhat == 0 everywhere"
        if training and track:
            rm, rv, nbt = N.bn_running64(N.bn_stats64(x, EPS), rm, rv, momentum, nbt)
            w.add(label + " running mean", tag, bn.running_mean, *rm, N.c_bn_mean(rows) + 8)
            w.add(label + " running var", tag, bn.running_var, *rv, N.c_bn_m2(rows) + 8)
            assert int(bn.num_batches_tracked) == nbt, tag
        if not track:
            assert bn.running_mean is None and bn.num_batches_tracked is None


@pytest.mark.parametrize("cols", [1, 3, 37, 64, 65, 100, 256, 400, 1030])
def test_batch_norm_rows_by_cols_against_float64(cols):
    """Rows 2 .. 1025 at every column count; randn, far-from-zero mean and constant columns."""
    w = Worst()
    for rows in SMALL_ROWS + ([8] if cols == 100 else []):
        for family in ("randn", "far_mean", "constant"):
            _bn_run(w, "bn W%d %s %s" % (bn_form(rows, cols)[:2] + (family,)), rows, cols, family)
    w.close()


def test_batch_norm_scalar_generic_loop_beyond_the_block_cap():
    w = Worst()
    for family in ("randn", "far_mean"):
        _bn_run(w, "bn cols 4099 generic " + family, 33, 4099, family)
    w.close()


@pytest.mark.parametrize("rows", BIG_ROWS)
def test_batch_norm_reduction_chains_against_float64(rows):
    w = Worst()
    for cols in (37, 100):
        for family in ("randn", "far_mean") + (("constant",) if rows in (30000, 32768) else ()):
            _bn_run(w, "bn rows %d %s" % (rows, family), rows, cols, family, steps=1)
    w.close()


@pytest.mark.parametrize("rows,cols", [(33000, 97), (131072, 100)])
def test_batch_norm_on_a_capped_grid_runs_the_unrolled_bodies(rows, cols):
    assert bn_form(rows, cols)[1:] == ("fixed", True, True)
    w = Worst()
    _bn_run(w, "bn capped W%d" % bn_form(rows, cols)[0], rows, cols, "randn", steps=1)
    w.close()


VARIANT_SHAPES = [(8, 100), (300, 100), (33, 37), (300, 37), (65, 64), (1025, 400)]
VARIANTS = {
    "relu": dict(act="relu"), "prelu1": dict(act="prelu1"), "preluC": dict(act="preluC"),
    "no affine": dict(affine_=False), "no affine relu": dict(affine_=False, act="relu"),
    "no running stats": dict(track=False), "no running stats preluC": dict(track=False, act="preluC"),
    "momentum None": dict(momentum=None), "no dx": dict(x_grad=False), "no dx relu": dict(x_grad=False, act="relu"),
    "no dx preluC": dict(x_grad=False, act="preluC"),
}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_batch_norm_variants_against_float64(variant):
    """Both loop bodies of both VEC forms (8 and 300 rows at cols 100; 33 and 300 at cols 37), two row blocks, many column
    blocks; every ReLU / PReLU case on sign-safe inputs and on the gamma == 0 family, whose columns stay in every
    comparison (z == beta there: beta == 0 takes the slope side, y == 0 exactly)."""
    kw = VARIANTS[variant]
    assert {bn_form(r, c)[:2] for r, c in VARIANT_SHAPES} == {(4, "generic"), (4, "fixed"), (1, "generic"), (1, "fixed")}
    w = Worst()
    for rows, cols in VARIANT_SHAPES:
        fams = ("randn", "far_mean") + (("gamma0",) if kw.get("affine_", True) else ())
        for family in fams:
            _bn_run(w, "bn %s %s" % (variant, family), rows, cols, family, seed=1, **kw)
    w.close()


@pytest.mark.parametrize("act", ["relu", "prelu1", "preluC"])
def test_batch_norm_activation_with_xhat_zero_and_beta_zero(act):
    """Constant columns behind an activation, gamma != 0, beta == 0 in every other column: xhat == 0 in every element, so
    z == beta exactly in all three kernels that recompute its sign (apply, backward partial, backward dx), and z == 0 takes
    the slope side.  No element is kept away from zero here; y is act(beta) exactly, dgamma exactly zero, and dbeta, dslope
    and dx meet their bounds with every column in the comparison.  (Training steps only: in evaluation mode z is no longer
    beta and nothing keeps it from the edge.)"""
    w = Worst()
    for rows, cols in VARIANT_SHAPES:
        _bn_run(w, "bn xhat == 0 " + act, rows, cols, "constant", act=act, eval_=False)
    w.close()


def test_batch_norm_refuses_one_row_in_training_as_torch_does():
    from recbox_amd import ops
    bn = nn.BatchNorm1d(5).cuda().train()
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        ops.batch_norm(torch.zeros(1, 5, device="cuda"), bn)
    torch.cuda.synchronize()
    bn.eval()
    assert tuple(ops.batch_norm(torch.zeros(1, 5, device="cuda"), bn).shape) == (1, 5)


# ---- the C entry points: statistics as they come out, the split entry points, alignment ---------------------------------------
def _ws(rows, cols):
    from recbox_amd import _lib
    n = _lib.lib.rbx_batchnorm_workspace_size(rows, cols)
    return torch.empty(max(n, 1), dtype=torch.uint8, device="cuda"), n


@pytest.mark.parametrize("rows", SMALL_ROWS + BIG_ROWS)
def test_batch_norm_statistics_against_float64(rows):
    """mean / rstd of rbx_batchnorm_fwd and the raw (n, mean, M2) of rbx_batchnorm_stats; on constant columns the mean is the
    constant and M2 zero, exactly."""
    from recbox_amd import _lib
    w = Worst()
    for cols in (37, 100):
        for family in ("randn", "far_mean", "constant"):
            x = FAMILIES[family]((rows, cols), rows + cols)
            xc = x.cuda()
            y, mean, rstd = torch.empty_like(xc), torch.empty(cols, device="cuda"), torch.empty(cols, device="cuda")
            rm, rv = torch.zeros(cols, device="cuda"), torch.ones(cols, device="cuda")
            ws, nws = _ws(rows, cols)
            _lib.check(_lib.lib.rbx_batchnorm_fwd(P(xc), rows, cols, None, None, EPS, 1, 0.1, P(rm), P(rv), 0, P(mean), P(rstd),
                                                  P(y), P(ws), nws, None))
            raw = torch.empty(3, cols, device="cuda")
            _lib.check(_lib.lib.rbx_batchnorm_stats(P(xc), rows, cols, P(raw), P(ws), nws, None))
            torch.cuda.synchronize()
            st = N.bn_stats64(x, EPS)
            tag = "[%d, %d] %s" % (rows, cols, family)
            label = "bn stats " + family
            w.add(label + " mean", tag, mean, *st["mean"], N.c_bn_mean(rows))
            w.add(label + " rstd", tag, rstd, *st["rstd"], N.c_bn_m2(rows))
            w.add(label + " raw mean", tag, raw[1], *st["mean"], N.c_bn_mean(rows))
            w.add(label + " raw M2", tag, raw[2], *st["m2"], N.c_bn_m2(rows))
            assert bool((raw[0] == float(rows)).all()), tag
            assert torch.equal(raw[1], mean), tag
            # the apply pass alone, the kernel's own statistics handed to the restatement: the floor
            w.add(label + " y given the statistics", tag, y, *N.bn_fwd64(x, None, None, EPS, mean=mean, rstd=rstd)["y"], N.C_BOUND)
            if family == "constant":
                assert torch.equal(mean.cpu(), x[0]) and int(torch.count_nonzero(raw[2])) == 0, tag
                assert int(torch.count_nonzero(y)) == 0, tag
    w.close()


@pytest.mark.parametrize("chunk", [1, 65, 4097])
@pytest.mark.parametrize("W", [2, 3])
def test_split_entry_points_merge_to_the_whole_batch(W, chunk):
    """rbx_batchnorm_stats / _apply / _bwd_reduce / _bwd_dx on W row chunks of one batch, merged in float64 as _SyncBatchNorm
    merges the ranks, against bn_fwd64 / bn_bwd64 of the whole batch (fused ReLU, sign-safe inputs)."""
    from recbox_amd import _lib
    lib = _lib.lib
    w = Worst()
    rows = W * chunk
    for cols in (37, 100):
        for family in ("randn", "far_mean"):
            gamma, beta = affine(cols, cols)
            C = N.c_bn_y(chunk)
            relu = chunk > 1          # (two or three rows: xhat is +-1 or so whatever x is, no move of x takes z from zero)
            x = FAMILIES[family]((rows, cols), rows + cols)
            if relu:
                x = sign_safe(x, gamma, beta, EPS, C)
            dy = randn((rows, cols), 3)
            gc, bc = gamma.cuda(), beta.cuda()
            parts = [x[k * chunk:(k + 1) * chunk].contiguous().cuda() for k in range(W)]
            dparts = [dy[k * chunk:(k + 1) * chunk].contiguous().cuda() for k in range(W)]
            ws, nws = _ws(chunk, cols)
            raws = []
            for xc in parts:
                raw = torch.empty(3, cols, device="cuda")
                _lib.check(lib.rbx_batchnorm_stats(P(xc), chunk, cols, P(raw), P(ws), nws, None))
                raws.append(raw.double())
            allraw = torch.stack(raws)
            n, mean_r, m2_r = allraw[:, 0], allraw[:, 1], allraw[:, 2]
            total = n.sum(0)
            mean64 = (n * mean_r).sum(0) / total
            m2 = m2_r.sum(0) + (n * (mean_r - mean64) ** 2).sum(0)
            mean, rstd = mean64.float(), torch.rsqrt(m2 / total + EPS).float()
            st = N.bn_stats64(x, EPS)
            tag = "W%d chunk %d cols %d %s" % (W, chunk, cols, family)
            label = "bn split " + family
            assert bool((total == rows).all()), tag
            w.add(label + " mean", tag, mean64, *st["mean"], N.c_bn_mean(chunk))
            w.add(label + " M2", tag, m2, *st["m2"], N.c_bn_m2(chunk))
            f = N.bn_fwd64(x, gamma, beta, EPS, relu=relu)
            ys, sums = [], []
            for xc, dc in zip(parts, dparts):
                y = torch.empty_like(xc)
                _lib.check(lib.rbx_batchnorm_apply(P(xc), chunk, cols, P(gc), P(bc), P(mean), P(rstd), int(relu), P(y), None))
                s = torch.empty(2, cols, device="cuda")
                _lib.check(lib.rbx_batchnorm_bwd_reduce(P(xc), P(dc), P(y) if relu else None, chunk, cols, P(mean), P(rstd), P(s[0]), P(s[1]),
                                                        P(ws), nws, None))
                ys.append(y), sums.append(s)
            glob = torch.stack(sums).double().sum(0).float()
            dxs = []
            for xc, dc, y in zip(parts, dparts, ys):
                dx = torch.empty_like(xc)
                _lib.check(lib.rbx_batchnorm_bwd_dx(P(xc), P(dc), P(y) if relu else None, chunk, cols, P(gc), P(mean), P(rstd), P(glob[0]), P(glob[1]),
                                                    rows, P(dx), None))
                dxs.append(dx)
            torch.cuda.synchronize()
            w.add(label + " y", tag, torch.cat(ys), *f["y"], N.c_bn_y(chunk))
            b = N.bn_bwd64(x, dy, gamma, f["mean"], f["rstd"], True, relu_mask=(f["y"][0] > 0) if relu else None)
            w.add(label + " dgamma", tag, glob[0], *b["dgamma"], N.c_bn_dgamma(chunk, chunk))
            w.add(label + " dbeta", tag, glob[1], *b["dbeta"], N.c_bn_sum(chunk))
            w.add(label + " dx", tag, torch.cat(dxs), *b["dx"], N.c_bn_dx(chunk, chunk))
    w.close()


@pytest.mark.parametrize("rows", [8, 300])
@pytest.mark.parametrize("which", ["all", "y_relu"])
def test_batch_norm_backward_takes_the_scalar_form_for_a_misaligned_operand(which, rows):
    """cols % 4 == 0 with x, dy, dx and y_relu at a storage offset of one float ("all"), and with y_relu alone there: the
    scalar form must run (bn_bwd_dx looked at x, dy and dx only and read a misaligned y_relu four at a time).  dx lies
    inside a NaN-filled wider buffer: nothing outside the block is written."""
    from recbox_amd import _lib
    lib = _lib.lib
    cols, n = 100, rows * 100
    w = Worst()
    gamma, beta = affine(cols, 5)
    x = sign_safe(FAMILIES["randn"]((rows, cols), rows), gamma, beta, EPS, N.c_bn_y(rows))
    dy = randn((rows, cols), 2)

    def at(t, off):
        buf = torch.full((n + 8,), float("nan"), device="cuda")
        buf[off:off + n] = t.reshape(-1).cuda()
        return buf, buf[off:off + n]

    o = 1 if which == "all" else 4
    (_, xc), (_, dc) = at(x, o), at(dy, o)
    ybuf, yv = at(torch.zeros(n), 1)
    dxbuf, dxv = at(torch.zeros(n), o)
    dxv.fill_(float("nan"))
    assert yv.data_ptr() % 16 == 4 and xc.data_ptr() % 16 == (4 if which == "all" else 0)
    gc, bc = gamma.cuda(), beta.cuda()
    mean, rstd = torch.empty(cols, device="cuda"), torch.empty(cols, device="cuda")
    rm, rv = torch.zeros(cols, device="cuda"), torch.ones(cols, device="cuda")
    ws, nws = _ws(rows, cols)
    _lib.check(lib.rbx_batchnorm_fwd(P(xc), rows, cols, P(gc), P(bc), EPS, 1, 0.1, P(rm), P(rv), 1, P(mean), P(rstd), P(yv),
                                     P(ws), nws, None))
    dg, db = torch.empty(cols, device="cuda"), torch.empty(cols, device="cuda")
    _lib.check(lib.rbx_batchnorm_bwd(P(xc), P(dc), P(yv), rows, cols, P(gc), P(mean), P(rstd), 1, P(dxv), P(dg), P(db), P(ws), nws,
                                     None))
    torch.cuda.synchronize()
    tag = "%s rows %d" % (which, rows)
    f = N.bn_fwd64(x, gamma, beta, EPS, relu=True)
    w.add("bn misaligned y", tag, yv.view(rows, cols), *f["y"], N.c_bn_y(rows))
    b = N.bn_bwd64(x, dy, gamma, f["mean"], f["rstd"], True, relu_mask=f["y"][0] > 0)
    w.add("bn misaligned dx", tag, dxv.view(rows, cols), *b["dx"], N.c_bn_dx(rows, rows))
    w.add("bn misaligned dgamma", tag, dg, *b["dgamma"], N.c_bn_dgamma(rows, rows))
    assert bool(torch.isnan(dxbuf[:o]).all()) and bool(torch.isnan(dxbuf[o + n:]).all()), "dx was written outside its block"
    assert bool(torch.isnan(ybuf[:1]).all()) and bool(torch.isnan(ybuf[1 + n:]).all()), "y was written outside its block"
    w.close()


@pytest.mark.parametrize("rows", [8, 300])
def test_batch_norm_prelu_entry_points_take_the_scalar_form_for_misaligned_operands(rows):
    """rbx_batchnorm_prelu_fwd / _bwd read x, dy and write y, dx four at a time (gamma, beta, slope and the statistics one at
    a time): all four at a storage offset of one float run the scalar form."""
    from recbox_amd import _lib
    lib = _lib.lib
    cols, n = 100, rows * 100
    w = Worst()
    gamma, beta = affine(cols, 6)
    sl = slopes(cols, True, 2)
    x = sign_safe(FAMILIES["randn"]((rows, cols), rows + 1), gamma, beta, EPS, N.c_bn_y(rows))
    dy = randn((rows, cols), 4)
    bufs = {}
    for name, t in (("x", x), ("dy", dy), ("y", None), ("dx", None)):
        buf = torch.full((n + 8,), float("nan"), device="cuda")
        if t is not None:
            buf[1:1 + n] = t.reshape(-1).cuda()
        bufs[name] = buf
    v = {k: b[1:1 + n] for k, b in bufs.items()}
    gc, bc, sc = gamma.cuda(), beta.cuda(), sl.cuda()
    mean, rstd = torch.empty(cols, device="cuda"), torch.empty(cols, device="cuda")
    rm, rv = torch.zeros(cols, device="cuda"), torch.ones(cols, device="cuda")
    ws, nws = _ws(rows, cols)
    _lib.check(lib.rbx_batchnorm_prelu_fwd(P(v["x"]), rows, cols, P(gc), P(bc), P(sc), cols, EPS, 1, 0.1, P(rm), P(rv), P(mean),
                                           P(rstd), P(v["y"]), P(ws), nws, None))
    dg, db, ds = (torch.empty(cols, device="cuda") for _ in range(3))
    _lib.check(lib.rbx_batchnorm_prelu_bwd(P(v["x"]), P(v["dy"]), rows, cols, P(gc), P(bc), P(sc), cols, P(mean), P(rstd), 1,
                                           P(v["dx"]), P(dg), P(db), P(ds), P(ws), nws, None))
    torch.cuda.synchronize()
    tag = "rows %d" % rows
    f = N.bn_fwd64(x, gamma, beta, EPS, slope=sl)
    w.add("bn prelu misaligned y", tag, v["y"].view(rows, cols), *f["y"], N.c_bn_y(rows))
    b = N.bn_bwd64(x, dy, gamma, f["mean"], f["rstd"], True, slope=sl, beta=beta)
    w.add("bn prelu misaligned dx", tag, v["dx"].view(rows, cols), *b["dx"], N.c_bn_dx(rows, rows))
    w.add("bn prelu misaligned dslope", tag, ds, *b["dslope"], N.c_bn_dgamma(rows, rows))
    for name in ("y", "dx"):
        assert bool(torch.isnan(bufs[name][:1]).all()) and bool(torch.isnan(bufs[name][1 + n:]).all()), name
    w.close()


# ---- LayerNorm ---------------------------------------------------------------------------------------------------------------------
LN_VEC = [4, 8, 12, 16, 20, 32, 36, 64, 68, 128, 132, 200, 256, 260, 512, 516, 1000, 1024]
LN_SCALAR = [1, 2, 3, 7, 10, 17, 33, 63, 65, 127, 129, 255]


def _ln_run(w, label, rows, dim, family, eps=1e-8, affine_="both", x_grad=True, fused=None, seed=0):
    from recbox_amd import ops
    gamma, beta = affine(dim, dim + seed)
    kw = {}
    if affine_ == "none":
        gamma = beta = None
        kw["elementwise_affine"] = False
    elif affine_ == "no_bias":
        beta = None
        kw["bias"] = False
    ln = nn.LayerNorm(dim, eps=eps, **kw).cuda()
    with torch.no_grad():
        if gamma is not None:
            ln.weight.copy_(gamma.cuda())
        if beta is not None:
            ln.bias.copy_(beta.cuda())
    x = ROW_FAMILIES[family]((rows, dim), rows + dim + seed)
    dy = randn((rows, dim), 3 + seed)
    xc = x.cuda().requires_grad_(x_grad)
    y = ops.layer_norm(xc, ln)
    y.backward(dy.cuda())
    torch.cuda.synchronize()
    tag = "[%d, %d] %s eps %g %s" % (rows, dim, family, eps, affine_)
    f = N.ln_fwd64(x, gamma, beta, eps)
    w.add(label + " y", tag, y, *f["y"], N.c_ln_y(dim))
    b = N.ln_bwd64(x, dy, gamma, eps)
    if x_grad:
        w.add(label + " dx", tag, xc.grad, *b["dx"], N.c_ln_dx(dim))
    else:
        assert xc.grad is None
    fused = x_grad if fused is None else fused
    if gamma is not None:
        w.add(label + " dgamma", tag, ln.weight.grad, *b["dgamma"], N.c_ln_sum(rows, dim, fused) + N.c_ln_stat(dim) + 8)
    if beta is not None:
        w.add(label + " dbeta", tag, ln.bias.grad, *b["dbeta"], N.c_ln_sum(rows, dim, fused))


@pytest.mark.parametrize("dim", LN_VEC + LN_SCALAR)
def test_layer_norm_at_every_form_against_float64(dim):
    w = Worst()
    label = "ln<%d, %d, %s>" % N.ln_form(dim)
    for rows in (1, 7, 257) + ((5000,) if dim in (64, 7) else ()):
        for family in ("randn", "far_mean", "constant"):
            for eps in (1e-8, 1e-5):
                _ln_run(w, "%s %s" % (label, family), rows, dim, family, eps)
    for affine_ in ("none",) + (("no_bias",) if "bias" in nn.LayerNorm.__init__.__code__.co_varnames else ()):
        _ln_run(w, "%s %s" % (label, affine_), 7, dim, "randn", affine_=affine_)
    for rows in (3, 2500):                      # parameter gradients only: one and three blocks of 1024 rows, the last ragged
        _ln_run(w, label + " parameter gradients only", rows, dim, "randn", x_grad=False)
    w.close()


def test_layer_norm_fused_parameter_gradients_past_the_workgroup_cap():
    """(300000, 16): the dx kernel that also leaves the partials is capped at 4 x CUs = 1024 workgroups."""
    w = Worst()
    _ln_run(w, "ln fused past the cap", 300000, 16, "randn")
    w.close()


@pytest.mark.parametrize("dim", [257, 1023, 1025, 1028])
def test_layer_norm_dims_without_a_form_are_refused(dim):
    """The kernel has no form beyond 256 lane slots: RBX_ERR_UNSUPPORTED from the C entry point, NotImplementedError from
    ops.layer_norm (nn.LayerNorm, the reference's module, has no such limit).  The call after the refusal runs."""
    from recbox_amd import _lib, ops
    x = randn((5, dim), dim).cuda()
    y, mean, rstd = torch.empty_like(x), torch.empty(5, device="cuda"), torch.empty(5, device="cuda")
    assert _lib.lib.rbx_layernorm_fwd(P(x), 5, dim, None, None, 1e-5, P(mean), P(rstd), P(y), None) == _lib.RBX_ERR_UNSUPPORTED
    with pytest.raises(NotImplementedError, match="layernorm: dim %d too large for one lane group" % dim):
        ops.layer_norm(x, nn.LayerNorm(dim).cuda())
    torch.cuda.synchronize()
    w = Worst()
    _ln_run(w, "ln after a refusal", 7, 64, "randn")
    w.close()


@pytest.mark.parametrize("dim", [1, 7, 16, 64, 255, 1024])
def test_layer_norm_row_statistics_against_float64(dim):
    from recbox_amd import _lib
    w = Worst()
    for family in ("randn", "far_mean", "constant"):
        rows = 61
        x = ROW_FAMILIES[family]((rows, dim), dim)
        xc = x.cuda()
        y, mean, rstd = torch.empty_like(xc), torch.empty(rows, device="cuda"), torch.empty(rows, device="cuda")
        _lib.check(_lib.lib.rbx_layernorm_fwd(P(xc), rows, dim, None, None, 1e-8, P(mean), P(rstd), P(y), None))
        torch.cuda.synchronize()
        f = N.ln_fwd64(x, None, None, 1e-8)
        w.add("ln mean " + family, "dim %d" % dim, mean, *f["mean"], N.C_BOUND)
        w.add("ln rstd " + family, "dim %d" % dim, rstd, *f["rstd"], N.c_ln_y(dim))
    w.close()


# ---- Dice and the stand-alone PReLU ---------------------------------------------------------------------------------------------------
ACT_ROWS = SMALL_ROWS + [7300, 16000, 30000, 32767, 32768]


def _act_shapes(cols):
    return [r for r in ACT_ROWS if r <= 1025 or cols in (37, 64, 65)]


@pytest.mark.parametrize("cols", [1, 3, 37, 64, 65, 256, 400])
def test_dice_against_float64(cols):
    """Training (two steps of the running statistics) and evaluation; alpha of either sign and alpha == 1."""
    from recbox_amd import ops
    w = Worst()
    for rows in _act_shapes(cols):
        for family in ("randn", "far_mean", "constant"):
            bn = nn.BatchNorm1d(cols, affine=False, eps=1e-9, momentum=0.01).cuda()
            alpha = nn.Parameter(dice_alpha(cols, cols).cuda())
            zero, one = torch.zeros(cols, dtype=torch.float64), torch.ones(cols, dtype=torch.float64)
            rm, rv, nbt = (zero, zero), (one, one), 0
            for step in range(2):
                training = step == 0
                bn.train(training)
                x = FAMILIES[family]((rows, cols), rows + cols + step)
                dy = randn((rows, cols), step)
                mean = rstd = None
                if not training:
                    mean = bn.running_mean.detach().cpu().double()
                    rstd = 1.0 / torch.sqrt(bn.running_var.detach().cpu().double() + N.f32(1e-9))
                xc = x.cuda().requires_grad_(True)
                alpha.grad = None
                y = ops.dice(xc, bn, alpha)
                y.backward(dy.cuda())
                torch.cuda.synchronize()
                tag = "[%d, %d] %s %s" % (rows, cols, family, "training" if training else "eval")
                label = "dice %s %s" % (family, "training" if training else "eval")
                w.add(label + " y", tag, y, *N.dice_fwd64(x, alpha, 1e-9, mean, rstd), N.c_dice_y(rows))
                b = N.dice_bwd64(x, dy, alpha, mean, rstd, training, 1e-9)
                w.add(label + " dx", tag, xc.grad, *b["dx"], N.c_dice_bwd(rows))
                w.add(label + " dalpha", tag, alpha.grad, *b["dalpha"], N.c_dice_bwd(rows))
                if training:
                    rm, rv, nbt = N.bn_running64(N.bn_stats64(x, 1e-9), rm, rv, 0.01, nbt)
                    w.add("dice running mean", tag, bn.running_mean, *rm, max(N.C_BOUND, 6 * N.act_depth(rows)))
                    w.add("dice running var", tag, bn.running_var, *rv, max(N.C_BOUND, 6 * N.act_depth(rows)))
                    assert int(bn.num_batches_tracked) == nbt
    w.close()


@pytest.mark.parametrize("cols", [1, 3, 37, 64, 65, 256, 400, 255, 257, 1030])
def test_standalone_prelu_against_float64(cols):
    """y and dx are one rounded product: equality.  The slope gradient per column (n_slope == cols) and summed over all
    columns by colsum_final_kernel's single workgroup (n_slope == 1; cols 1, 255, 256, 257, 1030 around its 256 lanes)."""
    from recbox_amd import ops
    w = Worst()
    for rows in ((65, 1025) if cols in (255, 257, 1030) else _act_shapes(cols)):
        for n_slope in (1, cols):
            x = randn((rows, cols), rows + cols)
            x[0, 0] = 0.0                                                     # x == 0: the slope side, dy x == 0
            dy = randn((rows, cols), 9)
            pre = nn.PReLU(n_slope).cuda()
            with torch.no_grad():
                pre.weight.copy_(slopes(cols, n_slope > 1, 4)[:n_slope].cuda())
            xc = x.cuda().requires_grad_(True)
            y = ops.prelu(xc, pre)
            y.backward(dy.cuda())
            torch.cuda.synchronize()
            p = N.prelu64(x, pre.weight, dy)
            tag = "[%d, %d] n_slope %d" % (rows, cols, n_slope)
            w.equal("prelu y", tag, y.detach(), p["y"])
            w.equal("prelu dx", tag, xc.grad, p["dx"])
            w.add("prelu dslope %s" % ("per column" if n_slope > 1 else "one slope"), tag, pre.weight.grad,
                  *(p["dslope"] if (n_slope > 1 or cols == 1) else p["dslope_sum"]), N.c_prelu_dslope(rows, cols, n_slope))
    w.close()
