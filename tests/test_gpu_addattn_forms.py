"""The fused additive attention pooling (csrc/rbx_addattn.hip) at every form its host code dispatches, against the float64
restatement of tests/addattn64.py under the scale-aware bar of tests/fp32_bar.py: per tensor, max|got - want| <=
max(4 e32, 2e-6 max|want|) with e32 the error of the same restatement (addattn64.forward) run in float32 on the CPU.
Nothing the kernels return enters the bar.

Forms (tiles of 16 positions; ceil(max(D, H) / 16) wavefronts; grid = min(B, 2048) workgroups):
  addattn_fwd_kernel<8>  / addattn_bwd_kernel<8>    max(D, H) <= 32   (4, 4) the floor, (20, 12), (32, 32)
  addattn_fwd_kernel<16> / addattn_bwd_kernel<16>   max(D, H) <= 64   (16, 64) hidden > dim, (36, 32)
  addattn_fwd_kernel<32> / addattn_bwd_kernel<32>   max(D, H) > 64    (4, 128), (128, 4), (64, 68), (100, 100), (128, 128)
  hidden > dim: the wavefronts past dim / 16 own no column of dx; dim > hidden: those past hidden / 16 own no unit.
  L = 1, 15, 16, 17, 33 (below, at and past one and two tiles); B = 1, 37; with and without ctx, with and without mask.
  B = 2048, 2085, 4097 at (L, D, H) = (3, 8, 8) and (17, 20, 12): aa_grid caps the launch at 2048 workgroups, a workgroup
  walks up to three samples, dv is summed over a workgroup's samples and then over 2048 workspace rows (addattn_dv_kernel).
  A fully masked sample beside valid ones at eps = 1e-12: its alpha, out and gradients are exactly 0, and the other samples'
  results are the bits of the batch without it.
  x as a strided view of a wider block (through ops), d_out with a wider row stride (through the C ABI), the filler 1e30:
  the bits of the contiguous call.  d_dpre [B, L, H] (the transient the dense path forms dW from) against the hand-written
  restatement of tests/test_fp32_bar_host.py, which that file holds to addattn64's autograd.
A spy on ops.lib counts rbx_addattn_fwd / rbx_addattn_bwd: the kernels ran, not the ATen composition.

Measured on the MI355X, worst err / bar over all cases of this module (bar factor 4 everywhere):
  out 0.13, alpha 0.15, dx 0.40, dw 0.57, dctx 0.46, dv 0.35, d_dpre 0.19: the bar holds 1.7 to 8 times over.
Found by test_every_width_length_and_operand_form at B = 1 (one valid position, the exact dW / dctx / dv are 0, so the bar
is 0): the backward summed G over 64 lanes and g_l over 16, and g_l - G left 4e-8 .. 7e-7 in dW where float64 and plain
fp32 give 0.  rbx_addattn_bwd now sums G in g_l's order; test_one_valid_position_leaves_no_parameter_gradient pins it."""
import ctypes

import pytest
import torch

import addattn64
from fp32_bar import assert_bar, report

pytestmark = pytest.mark.gpu
SHAPES = [(4, 4), (16, 64), (4, 128), (128, 4), (20, 12), (32, 32), (36, 32), (64, 68), (100, 100), (128, 128)]
LENGTHS = [1, 15, 16, 17, 33]


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _fused(*a):
    from recbox_amd import ops
    return ops.additive_attn_pool(*a)


def _spy(monkeypatch):
    from recbox_amd import ops
    calls = []
    real = ops.lib

    class Spy(object):
        def rbx_addattn_fwd(self, *a):
            calls.append("fwd")
            return real.rbx_addattn_fwd(*a)

        def rbx_addattn_bwd(self, *a):
            calls.append("bwd")
            return real.rbx_addattn_bwd(*a)

        def __getattr__(self, name):
            return getattr(real, name)
    monkeypatch.setattr(ops, "lib", Spy())
    return calls


def _refs(case, **form):
    return addattn64.reference(case, **form), addattn64.run(addattn64.forward, case, "cpu", **form)


def _assert(got, want, ref32, tag, names=addattn64.NAMES):
    for n in names:
        if want[n] is None:
            assert got[n] is None, n
        else:
            assert_bar("%s %s" % (n, tag), got[n], want[n], ref32[n])


@pytest.mark.parametrize("D,H", SHAPES)
def test_every_width_length_and_operand_form(D, H, monkeypatch):
    calls = _spy(monkeypatch)
    runs = 0
    for B in (1, 37):
        for L in LENGTHS:
            case = addattn64.make_case(B, L, D, H, seed=30)
            forms = [(True, True)] + ([(False, True), (True, False), (False, False)] if L in (1, 17) else [])
            for use_ctx, masked in forms:
                form = dict(use_ctx=use_ctx, masked=masked)
                want, ref32 = _refs(case, **form)
                got = addattn64.run(_fused, case, "cuda", **form)
                _assert(got, want, ref32, "D=%d H=%d B=%d L=%d ctx=%d mask=%d" % (D, H, B, L, use_ctx, masked))
                runs += 1
    assert calls == ["fwd", "bwd"] * runs
    report("addattn D=%d H=%d" % (D, H))


@pytest.mark.parametrize("B", [2048, 2085, 4097])
@pytest.mark.parametrize("L,D,H", [(3, 8, 8), (17, 20, 12)])
def test_more_samples_than_workgroups(L, D, H, B, monkeypatch):
    """make_case scales the upstream gradient by 1 / sqrt(B); every tensor is compared whole, so the first, the middle and
    the last sample's dx and dctx are in."""
    calls = _spy(monkeypatch)
    case = addattn64.make_case(B, L, D, H, seed=31)
    want, ref32 = _refs(case)
    got = addattn64.run(_fused, case, "cuda")
    assert calls == ["fwd", "bwd"]
    tag = "B=%d L=%d D=%d H=%d" % (B, L, D, H)
    _assert(got, want, ref32, tag)
    for b in (0, B // 2, B - 1):
        for n in ("dx", "dctx"):
            assert_bar("%s[%d] %s" % (n, b, tag), got[n][b], want[n][b], ref32[n][b])
    report("addattn " + tag)


@pytest.mark.parametrize("L,D,H", [(17, 20, 12), (33, 36, 32), (16, 16, 64)])
def test_fully_masked_sample_beside_valid_ones(L, D, H, monkeypatch):
    calls = _spy(monkeypatch)
    B, dead, eps = 37, 5, 1e-12
    case = dict(addattn64.make_case(B, L, D, H, seed=32))
    case["mask"] = case["mask"].clone()
    case["mask"][dead] = 0
    want, ref32 = _refs(case, eps=eps)
    got = addattn64.run(_fused, case, "cuda", eps=eps)
    _assert(got, want, ref32, "masked sample L=%d D=%d H=%d" % (L, D, H))
    for n in ("alpha", "out", "dx", "dctx"):
        assert (got[n][dead] == 0).all(), n
    keep = torch.arange(B) != dead
    without = {k: (v[keep] if v.shape[:1] == (B,) else v) for k, v in case.items()}
    other = addattn64.run(_fused, without, "cuda", eps=eps)
    for n in ("alpha", "out", "dx", "dctx"):
        assert torch.equal(got[n][keep.to(got[n].device)], other[n]), n
    w2, r2 = _refs(without, eps=eps)
    _assert(other, w2, r2, "without the masked sample L=%d D=%d H=%d" % (L, D, H))
    assert calls == ["fwd", "bwd"] * 2
    report("addattn masked sample L=%d D=%d H=%d" % (L, D, H))


@pytest.mark.parametrize("L,D,H", [(17, 20, 12), (33, 100, 100), (16, 16, 64)])
def test_one_valid_position_leaves_no_parameter_gradient(L, D, H, monkeypatch):
    """alpha is exactly 1 there, so g_l - G must cancel to the bit (the backward sums G in the order it sums g_l): dW, dctx
    and dv are exactly 0 and dx is d_out at that position, 0 elsewhere -- as in float64 and in plain fp32."""
    calls = _spy(monkeypatch)
    B = 37
    case = dict(addattn64.make_case(B, L, D, H, seed=35))
    pos = torch.arange(B) % L
    case["mask"] = torch.zeros(B, L, dtype=torch.long)
    case["mask"][torch.arange(B), pos] = 1
    got = addattn64.run(_fused, case, "cuda")
    assert calls == ["fwd", "bwd"]
    for n in ("dw", "dctx", "dv"):
        assert torch.count_nonzero(got[n]) == 0, n
    expect = torch.zeros(B, L, D)
    expect[torch.arange(B), pos] = case["g_out"]
    assert torch.equal(got["dx"].cpu(), expect)
    want, ref32 = _refs(case)
    _assert(got, want, ref32, "one valid position L=%d D=%d H=%d" % (L, D, H))


@pytest.mark.parametrize("L,D,H", [(17, 20, 12), (33, 36, 64), (16, 128, 4)])
def test_strided_x_gives_the_contiguous_bits(L, D, H, monkeypatch):
    calls = _spy(monkeypatch)
    B = 37
    case = addattn64.make_case(B, L, D, H, seed=33)
    base = addattn64.run(_fused, case, "cuda")
    wide = torch.full((B, L + 3, D + 12), 1e30, device="cuda")
    wide[:, 1:L + 1, 8:8 + D] = case["x"].cuda()
    view = wide[:, 1:L + 1, 8:8 + D].detach().requires_grad_(True)
    assert not view.is_contiguous() and view.data_ptr() % 16 == 0
    got = addattn64.run(_fused, case, "cuda", x=view)
    assert calls == ["fwd", "bwd"] * 2                                          # the view is read in place, not refused
    for n in addattn64.NAMES:
        assert torch.equal(got[n], base[n]), n
    want, ref32 = _refs(case)
    _assert(got, want, ref32, "strided x L=%d D=%d H=%d" % (L, D, H))


@pytest.mark.parametrize("B,L,D,H", [(37, 17, 20, 12), (5, 33, 16, 64), (37, 16, 100, 100), (2085, 3, 8, 8)])
def test_c_abi_dpre_and_strided_d_out(B, L, D, H):
    from recbox_amd import _lib
    from test_fp32_bar_host import addattn_manual
    lib = _lib.lib
    case = addattn64.make_case(B, L, D, H, seed=34)
    x, w, c, v, g = (case[n].cuda() for n in ("x", "w", "ctx", "v", "g_out"))
    mask = case["mask"].cuda()
    nan = lambda *s: torch.full(s, float("nan"), device="cuda")
    out, alpha = nan(B, D), nan(B, L)
    rc = lib.rbx_addattn_fwd(_p(x), L * D, D, _p(w), _p(c), _p(v), _p(mask), _lib.RBX_I64, 0.0, B, L, D, H, _lib.RBX_F32, _p(out),
                             _p(alpha), None)
    assert rc == 0, _lib.last_error()
    ws_bytes = lib.rbx_addattn_bwd_workspace_size(B, H)
    assert ws_bytes == min(B, 2048) * H * 4

    def bwd(dout, stride):
        dx, dctx, dv, dpre = nan(B, L, D), nan(B, H), nan(H), nan(B, L, H)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
        rc = lib.rbx_addattn_bwd(_p(dout), stride, _p(x), L * D, D, _p(w), _p(c), _p(v), _p(mask), _lib.RBX_I64, _p(alpha), 0.0,
                                 B, L, D, H, _lib.RBX_F32, _p(dx), _p(dctx), _p(dv), _p(dpre), _p(ws), ws_bytes, None)
        assert rc == 0, _lib.last_error()
        torch.cuda.synchronize()
        return {"dx": dx, "dctx": dctx, "dv": dv, "dpre": dpre}
    plain = bwd(g, D)
    block = torch.full((B, D + 12), 1e30, device="cuda")
    block[:, :D] = g
    strided = bwd(block, D + 12)
    for n in plain:
        assert torch.equal(plain[n], strided[n]), n
    want, ref32 = addattn_manual(case, torch.float64), addattn_manual(case, torch.float32)
    tag = "c-abi B=%d L=%d D=%d H=%d" % (B, L, D, H)
    strided.update(out=out, alpha=alpha)
    for n in ("out", "alpha", "dx", "dctx", "dv", "dpre"):
        assert_bar("%s %s" % (n, tag), strided[n], want[n], ref32[n])
    auto = addattn64.reference(case)                                            # the hand-written float64 is the autograd one
    for n in ("dx", "dctx", "dv"):
        assert float((want[n] - auto[n]).abs().max()) <= 1e-12 * float(auto[n].abs().max())
    report("addattn " + tag)
