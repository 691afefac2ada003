"""The expert-gate mixing kernels (csrc/rbx_mix.hip: mix_fwd_kernel<NC>, mix_bwd_kernel<G, NC>) at every form the launchers
dispatch, against the restatement of tests/mix64.py under the scale-aware bar of tests/fp32_bar.py: per tensor max|got - want|
<= max(4 e32, 2e-6 max|want|), e32 the error of the same restatement (mix64.reference32) run in float32 on the CPU.  Nothing
the kernels return enters the bar, and the factor is 4 everywhere.

The forward uses __expf.  No additional term is given to p or out for it, and the kernel is unchanged: v_exp_f32 is good to
1 ulp and the fp32 product (z - max) log2(e) in front of it adds |z - max| 2^-24 relative, so p is off by at most
p |ln p| 2^-24 <= 2.2e-8 absolutely whatever the logits are (p |ln p| <= 1 / e), a hundredth of the floor 2e-6 max|p| of a
gate whose largest weight is O(1).  The measured ratios below agree.

Forms: a sample is owned by a lane group of G = 1, 2, 4, 4, 8, 16, 32, 64 lanes at H = 4, 8, 12, 16, 32, 64, 128, 256 (H = 12
leaves one lane of four idle), and from H = 260 on a lane owns NC = 2, 3, 4 float4 columns: H = 260, 516, 772 (NC = 4 with its
last column partly empty), 1024.  Per form B = 1, 37 and one sample more than a workgroup owns (4 * 64 / G + 1).  Selections
with n_t = 16 > G at H = 8, 12, 32: the lane that parks dp, pos & (G - 1), wraps and finishes several entries.  softmax on and
off.  Logits of +-80, and a peaked gate (one logit 20 above the rest in every sample: dz is about 1e-8 in size).  Experts,
logits and upstream gradients of size 0.1, 0.1, 1e-3 (mix64.small_wrap_case: the inputs of the host test's mutants).
Through the C ABI with NaN guards around every output: a gate with dout = NULL, dz = NULL, some dx[e] = NULL, experts read at a
row stride of E H (AITM's interleaved form: rows e of one [B, E, H] block).
``fused_only`` makes the composition raise: what passes through ops.expert_mix ran the kernels; the C ABI calls assert RBX_OK.

Measured on the MI355X, worst err / bar over all cases of this module (34 tests, 2.6 s): out 0.12, p 0.05, dx 0.12, dz 0.25
(the rows with logits of +-80, where the kernel's dz has the bits of the float32 restatement).  Every kernel holds the bar with
the factor 4, __expf included; nothing had to be fixed.
Mutation check (a scratch build, never committed): mix_bwd_kernel forming dX_e from p (1 - 1e-5) -- a relative error of 1e-5,
4e-5 at the largest element -- fails all 34 tests here and passes all 38 tests of tests/test_gpu_expert_mix.py."""
import ctypes

import pytest
import torch

import mix64
from fp32_bar import assert_bar, report
from guarded import Guarded, ptr as _p

pytestmark = pytest.mark.gpu
FORMS = [4, 8, 12, 16, 32, 64, 128, 256, 260, 516, 772, 1024]
PLE = mix64.ple_select(2, 2, 1)


@pytest.fixture
def fused_only(monkeypatch):
    """For the duration of the test the composition raises: what passes went through the kernels."""
    from recbox_amd import ops

    def refuse(*a, **k):
        raise AssertionError("expert_mix_torch was called: the fused path did not run")
    assert ops.config.expert_mix_fused
    monkeypatch.setattr(ops, "expert_mix_torch", refuse)


def _group(H):
    g = 1
    while g < min(H // 4, 64):
        g *= 2
    return g


def _assert(got, want, ref32, tag, keys=("out", "dx", "dz")):
    for key in keys:
        for i, (a, b, c) in enumerate(zip(got[key], want[key], ref32[key])):
            if a is not None:
                assert_bar("%s %s [%d]" % (key, tag, i), a, b, c)


def _check(case, softmax=True, tag=""):
    from recbox_amd import ops
    want, ref32 = mix64.reference(case, softmax), mix64.reference32(case, softmax)
    got = mix64.run(ops.expert_mix, case, "cuda", softmax)
    _assert(got, want, ref32, tag)
    return got


@pytest.mark.parametrize("H", FORMS)
def test_every_lane_group_and_column_form(H, fused_only):
    G = _group(H)
    for batch in (1, 37, 4 * 64 // G + 1):
        for softmax in (True, False):
            _check(mix64.make_case(H + batch, batch, H, 5, PLE), softmax, "H=%d B=%d softmax=%d" % (H, batch, softmax))
    report("mix H=%d" % H)


@pytest.mark.parametrize("H", [8, 12, 32])
def test_more_selected_experts_than_lanes_in_the_group(H, fused_only):
    """n_t = 16 > G = 2, 4, 8: lane pos & (G - 1) parks dp for several positions and rewrites each of them."""
    for softmax in (True, False):
        case = mix64.make_case(70 + H, 37, H, 16, mix64.full_select(16, 2) + [[15, 3, 9, 0, 12, 6, 1]])
        _check(case, softmax, "n=16 H=%d softmax=%d" % (H, softmax))
    _check(mix64.small_wrap_case(H), True, "small n=16 H=%d" % H)
    report("mix n=16 H=%d" % H)


@pytest.mark.parametrize("H", [4, 12, 64, 260, 772])
def test_small_upstream_gradient(H, fused_only):
    case = mix64.make_case(90 + H, 37, H, 5, PLE, up=1e-3)
    _check(case, True, "up=1e-3 H=%d" % H)
    _check(case, False, "up=1e-3 H=%d weights" % H)
    report("mix up=1e-3 H=%d" % H)


@pytest.mark.parametrize("H", [4, 12, 128, 516])
def test_extreme_and_peaked_logits(H, fused_only):
    case = mix64.make_case(7 + H, 37, H, 4, mix64.full_select(4, 2))
    case["z"][0][3] = torch.tensor([80.0, -80.0, 79.0, -80.0])
    case["z"][1][5] = torch.tensor([-80.0, -80.0, -80.0, 80.0])
    got = _check(case, True, "logits of +-80 H=%d" % H)
    assert all(bool(torch.isfinite(t).all()) for key in ("out", "dx", "dz") for t in got[key])
    peaked = mix64.make_case(8 + H, 37, H, 4, mix64.full_select(4, 2))
    for z in peaked["z"]:
        z[torch.arange(37), torch.arange(37) % 4] += 20.0
    want = mix64.reference(peaked)
    assert all(float(d.abs().max()) < 1e-5 for d in want["dz"])                     # far below what an absolute 1e-4 can see
    _check(peaked, True, "peaked gate H=%d" % H)
    report("mix logits H=%d" % H)


# ---- the C ABI, every output between guards -----------------------------------------------------------------------------------
def _c_abi(case, softmax, no_dout=(), no_dz=(), no_dx=(), interleave=False):
    """{"out", "p", "dx", "dz"} through rbx_expert_mix_fwd / _bwd.  ``no_dout``: gates whose upstream gradient is NULL;
    ``no_dz`` / ``no_dx``: gradients passed as NULL; ``interleave``: the experts are rows e of one [B, E, H] block (row stride
    E H).  Every output is checked for untouched guards."""
    from recbox_amd import _lib, ops
    lib = _lib.lib
    E, T = len(case["x"]), len(case["z"])
    Bn, H = case["x"][0].shape
    if interleave:
        block = torch.stack(case["x"], dim=1).cuda()
        xs_t, stride = [block[:, e] for e in range(E)], E * H
    else:
        xs_t, stride = [t.cuda() for t in case["x"]], H
    zs_t = [t.cuda() for t in case["z"]]
    ups = [t.cuda() for t in case["up"]]
    sel, off, offs = ops._mix_sel_arrays(case["select"])
    xs = (ctypes.c_void_p * E)(*[t.data_ptr() for t in xs_t])
    strides = (ctypes.c_int64 * E)(*[stride] * E)
    zs = (ctypes.c_void_p * T)(*[t.data_ptr() for t in zs_t])
    out = Guarded(T * Bn, H)
    p = Guarded(Bn, offs[-1]) if softmax else None
    rc = lib.rbx_expert_mix_fwd(xs, strides, zs, sel, off, Bn, H, E, T, int(softmax), _lib.RBX_F32, _p(out.view),
                                _p(p.view) if softmax else None, None)
    assert rc == _lib.RBX_OK, _lib.last_error()
    torch.cuda.synchronize()
    assert out.untouched() and (p is None or p.untouched())
    dx = [None if e in no_dx else Guarded(Bn, H) for e in range(E)]
    dz = [None if t in no_dz else Guarded(Bn, offs[t + 1] - offs[t]) for t in range(T)]
    gs = (ctypes.c_void_p * T)(*[None if t in no_dout else ups[t].data_ptr() for t in range(T)])
    dxs = (ctypes.c_void_p * E)(*[None if g is None else g.view.data_ptr() for g in dx])
    dzs = (ctypes.c_void_p * T)(*[None if g is None else g.view.data_ptr() for g in dz])
    rc = lib.rbx_expert_mix_bwd(xs, strides, zs, _p(p.view) if softmax else None, gs, sel, off, Bn, H, E, T, int(softmax),
                                _lib.RBX_F32, dxs, dzs, None)
    assert rc == _lib.RBX_OK, _lib.last_error()
    torch.cuda.synchronize()
    for g in dx + dz + [out] + ([p] if softmax else []):
        assert g is None or g.untouched(), "a guard band was written"
    ps = [p.view[:, offs[t]:offs[t + 1]] for t in range(T)] if softmax else [None] * T
    return {"out": [out.view[t * Bn:(t + 1) * Bn] for t in range(T)], "p": ps,
            "dx": [None if g is None else g.view for g in dx], "dz": [None if g is None else g.view for g in dz]}


@pytest.mark.parametrize("softmax", [True, False])
@pytest.mark.parametrize("H", [4, 12, 32, 256, 772])
def test_c_abi_null_gradients_and_interleaved_rows(H, softmax):
    case = mix64.make_case(20 + H, 37, H, 5, PLE)
    used = {0, 2}
    want, ref32 = mix64.reference(case, softmax, used), mix64.reference32(case, softmax, used)
    tag = "c-abi H=%d softmax=%d" % (H, softmax)
    keys = ("out", "p", "dx", "dz") if softmax else ("out", "dx", "dz")
    got = _c_abi(case, softmax, no_dout={1})
    _assert(got, want, ref32, tag + " dout[1]=NULL", keys)
    assert float(got["dz"][1].abs().max()) == 0.0                               # a gate without gradient: zeros, written
    full = mix64.reference(case, softmax), mix64.reference32(case, softmax)
    got = _c_abi(case, softmax, no_dz={0, 2}, no_dx={1, 4})
    _assert(got, full[0], full[1], tag + " dz / dx NULLs", keys)
    got = _c_abi(case, softmax, no_dz={0, 1, 2})
    _assert(got, full[0], full[1], tag + " no dz", keys)
    got = _c_abi(case, softmax, interleave=True)
    _assert(got, full[0], full[1], tag + " interleaved", keys)
    plain = _c_abi(case, softmax)
    for key in keys:
        for a, b in zip(got[key], plain[key]):
            assert torch.equal(a, b), key                                        # the stride changes no bit
    report("mix " + tag)
