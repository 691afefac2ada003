"""The multi-interest capsule kernels (csrc/rbx_capsule.hip) at every form their host code dispatches, against the float64
restatement of tests/capsule64.py under the scale-aware bar of tests/fp32_bar.py: per tensor, max|got - want| <=
max(4 e32, 2e-6 max|want|) with e32 the error of the same restatement run in float32 on the CPU.  Nothing the kernels return
enters the bar.

Forms (N = K D; D a multiple of 4 in 4 .. 128, K in 1 .. 32):
  capsule_hat_kernel         (128 samples, position) per workgroup, W_l in slices of 64 of its N rows: N = 4 (below one slice),
                             N = 96 / 108 / 136 / 140 / 100 (a ragged last slice), N = 128 / 256 (whole slices); K = 32 at D = 4
  capsule_route_kernel       min(4, 16000 / slab) tasks (b, k) per workgroup, slab = L (D + 4) + D floats: 4, 3, 2 and 1 tasks,
                             each with a task count that is no multiple of it; the largest [L, D] slab
                             rbx_capsule_route_supported admits at D = 64 and D = 128, and the refusal one position further
  capsule_ds_kernel          ds alone (the fused op), ds and the stored d_hat (capsule_bilinear + capsule_route as two ops),
                             d_hat summed over k for the shared hat of type 0
  capsule_dx_kernel<NT> / capsule_dw_kernel<NT>   NT = ceil(D / 32) column blocks: <1> D = 4, 20, 32; <2> D = 36, 64;
                             <3> D = 68, 96; <4> D = 100, 128; a ragged last 32-step of dx (N = 36, 100, 108, 140), a ragged
                             last 128-row tile of dW (D = 20, K = 7: N = 140; N = 136)
  B = 1, 128, 129, 301 (below, at and past one 128-sample tile, three tiles) and L = 1, 63, 64, 65
  bilinear types 0 (shared hat, random start), 1 and 2; routing_times 3 and 5
A spy on ops.lib records which entry points ran.

Measured on the MI355X, worst err / bar over all cases of this module (bar factor 4 everywhere):
  type 2, one op    out 0.52, dx 0.62, dW 0.50 (all three at D = 96, K = 1; below 0.47 everywhere else)
  type 2, two ops   out 0.31, dx 0.34, dW 0.27
  types 0 and 1     out 0.30, dx 0.31, dW 0.40
  largest slab      out 0.31, dx 0.31, dW 0.22; the refused L + 1 on the composition stays below 0.2
  the bar holds 1.6 to 10 times over."""
import ctypes

import pytest
import torch

from fp32_bar import assert_bar, report
from test_gpu_capsule import _composition, _fused, _inputs, _run, _split

pytestmark = pytest.mark.gpu
WG_FLOATS = 16000                 # kCapWgFloats: the LDS floats of a routing workgroup
ENTRY = ("rbx_capsule_hat", "rbx_capsule_route_fwd", "rbx_capsule_route_bwd", "rbx_capsule_bilinear_dx",
         "rbx_capsule_bilinear_dw")
FUSED_CALLS = ["hat", "route_fwd", "route_bwd", "bilinear_dx", "bilinear_dw"]


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _spy(monkeypatch):
    from recbox_amd import ops
    calls = []
    real = ops.lib

    class Spy(object):
        def __getattr__(self, name):
            fn = getattr(real, name)
            if name not in ENTRY:
                return fn

            def counted(*a):
                calls.append(name[len("rbx_capsule_"):])
                return fn(*a)
            return counted
    monkeypatch.setattr(ops, "lib", Spy())
    return calls


def _tasks_per_workgroup(L, D):
    return max(1, min(4, WG_FLOATS // (L * (D + 4) + D)))


def _check(btype, B, L, D, K, fn=_fused, seed=40, rt=3, scale=1.0):
    x, w, mask, init, r = _inputs(btype, B, L, D, K, seed, scale)
    want = _run(_composition, x, w, mask, init, r, btype, K, "cpu", torch.float64, rt)
    ref32 = _run(_composition, x, w, mask, init, r, btype, K, "cpu", torch.float32, rt)
    got = _run(fn, x, w, mask, init, r, btype, K, "cuda", torch.float32, rt)
    tag = "type %d B=%d L=%d D=%d K=%d rt=%d" % (btype, B, L, D, K, rt)
    for what, a, b, c in zip(("out", "dx", "dW"), got, want, ref32):
        assert a is not None, what
        assert_bar("%s %s" % (what, tag), a, b, c)
    return got


# D, K: every NT of the dx / dW GEMMs on both sides of its boundaries, N from 4 to 256
WIDTHS = [(4, 1), (4, 32), (20, 7), (32, 3), (36, 1), (36, 3), (64, 2), (68, 2), (96, 1), (100, 1), (128, 2)]
# every B with every L once, and the corners twice
BATCH_LENGTH = [(1, 1), (128, 63), (129, 64), (301, 65), (1, 65), (301, 1), (128, 64), (129, 63)]


@pytest.mark.parametrize("D,K", WIDTHS)
def test_bilinear_route_at_every_width_batch_and_length(D, K, monkeypatch):
    from recbox_amd import ops
    calls = _spy(monkeypatch)
    for B, L in BATCH_LENGTH:
        assert ops.capsule_supported(L, D, K)
        _check(2, B, L, D, K)
    assert calls == FUSED_CALLS * len(BATCH_LENGTH)
    report("capsule type 2 D=%d K=%d" % (D, K))


@pytest.mark.parametrize("per,B,L,D,K", [(4, 37, 7, 16, 3), (3, 37, 70, 64, 2), (2, 37, 100, 64, 1), (1, 5, 130, 64, 3)])
def test_tasks_per_routing_workgroup(per, B, L, D, K, monkeypatch):
    """4, 3, 2 and 1 tasks per workgroup; the last workgroup is partly idle (B K is no multiple of the count)."""
    calls = _spy(monkeypatch)
    assert _tasks_per_workgroup(L, D) == per and (per == 1 or (B * K) % per != 0)
    _check(2, B, L, D, K, seed=41)
    assert calls == FUSED_CALLS
    report("capsule %d tasks per workgroup" % per)


def _largest_length(D):
    from recbox_amd import _lib
    L = 1
    while _lib.lib.rbx_capsule_route_supported(L + 1, D):
        L += 1
    return L


@pytest.mark.parametrize("D,expect", [(64, 209), (128, 107)])
def test_largest_slab_and_the_refusal_past_it(D, expect, monkeypatch):
    """cap_slab(L, D) = L (D + 1) + 3 L + D <= 14336 floats: L <= (14336 - D) / (D + 4), 209 at D = 64 and 107 at D = 128.
    L + 1: the entry point refuses by status code, the layer runs the einsum composition, within the same bar."""
    from recbox_amd import _lib, ops
    from recbox_amd.rechub.basic.layers import CapsuleNetwork
    L = _largest_length(D)
    assert L == expect
    B, K = 5, 1
    calls = _spy(monkeypatch)
    _check(2, B, L, D, K, seed=42)
    assert calls == FUSED_CALLS
    assert not ops.capsule_supported(L + 1, D, K)
    hat = torch.zeros(B, L + 1, K * D, device="cuda")
    mask = torch.ones(B, L + 1, dtype=torch.long, device="cuda")
    v, c, s = (torch.full(sh, float("nan"), device="cuda") for sh in ((B, K, D), (B, K, L + 1), (B, K, D)))
    rc = _lib.lib.rbx_capsule_route_fwd(_p(hat), (L + 1) * K * D, D, K * D, _p(mask), _lib.RBX_I64, L + 1, 1, None, B, K, L + 1, D,
                                        2, _p(v), _p(c), _p(s), None)
    assert rc == _lib.RBX_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.isnan(v).all()                                                 # nothing was launched
    del calls[:]
    x, w, mask, init, r = _inputs(2, B, L + 1, D, K, 42)
    want = _run(_composition, x, w, mask, init, r, 2, K, "cpu", torch.float64)
    ref32 = _run(_composition, x, w, mask, init, r, 2, K, "cpu", torch.float32)
    cap = CapsuleNetwork(D, L + 1, bilinear_type=2, interest_num=K).cuda()
    with torch.no_grad():
        cap.w.copy_(w)
    xg = x.cuda().requires_grad_(True)
    out = cap(xg, mask.cuda())
    out.backward(r.cuda().float())
    assert calls == []                                                          # the composition, no capsule kernel
    for what, a, b, c in zip(("out", "dx", "dW"), (out, xg.grad, cap.w.grad), want, ref32):
        assert_bar("%s refused L=%d D=%d" % (what, L + 1, D), a, b, c)
    report("capsule largest slab D=%d" % D)


@pytest.mark.parametrize("btype", [0, 1])
@pytest.mark.parametrize("B,L,D,K", [(129, 7, 16, 4), (37, 65, 36, 3), (301, 33, 68, 2), (1, 1, 4, 32), (128, 64, 128, 2)])
def test_linear_forms(btype, B, L, D, K, monkeypatch):
    """Type 0: one [B, L, D] hat every interest reads (hat_stride_k = 0), a random start, d_hat summed over k in order.
    Type 1: hat [B, L, K D] from one Linear.  Both: ops.linear, then rbx_capsule_route_fwd / _bwd with a stored d_hat."""
    calls = _spy(monkeypatch)
    _check(btype, B, L, D, K, seed=43)
    assert calls == ["route_fwd", "route_bwd"]
    report("capsule type %d D=%d" % (btype, D))


@pytest.mark.parametrize("btype,B,L,D,K", [(2, 129, 7, 20, 7), (2, 37, 64, 64, 2), (0, 37, 17, 36, 3)])
def test_routing_times_3_and_5(btype, B, L, D, K, monkeypatch):
    """Nothing is updated after iteration 2: five routing times are the three, to the bit."""
    calls = _spy(monkeypatch)
    three = _check(btype, B, L, D, K, seed=44, rt=3)
    five = _check(btype, B, L, D, K, seed=44, rt=5)
    for a, b in zip(three, five):
        assert torch.equal(a, b)
    assert calls == (FUSED_CALLS if btype == 2 else ["route_fwd", "route_bwd"]) * 2
    report("capsule routing times type %d" % btype)


@pytest.mark.parametrize("B,L,D,K", [(129, 7, 20, 7), (301, 63, 36, 3), (128, 65, 68, 2), (1, 1, 4, 1), (37, 33, 100, 1),
                                     (129, 64, 128, 2)])
def test_bilinear_and_route_as_two_ops(B, L, D, K, monkeypatch):
    """ops.capsule_bilinear + ops.capsule_route: capsule_ds_kernel stores d_hat [B, L, K D], the dx / dW GEMMs read it with
    c = NULL (gs_b = L N, gs_l = N)."""
    calls = _spy(monkeypatch)
    two = _check(2, B, L, D, K, fn=_split, seed=45)
    assert calls == ["hat", "route_fwd", "route_bwd", "bilinear_dx", "bilinear_dw"]
    del calls[:]
    one = _check(2, B, L, D, K, seed=45)
    assert torch.equal(one[0], two[0])                                          # the same forward kernels
    report("capsule two ops D=%d K=%d" % (D, K))
