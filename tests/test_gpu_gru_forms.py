"""The fused GRU recurrence (csrc/rbx_gru.hip) at every form its host code dispatches, against the float64 restatement of
tests/gru64.py under the scale-aware bar of tests/fp32_bar.py: per tensor, max|got - want| <= max(4 e32, 2e-6 max|want|) with
e32 the error of the same restatement run in float32 on the CPU.  Nothing the kernel returns enters the bar.

Forms (workgroup = 16 samples, one wavefront per 16 hidden units, H a multiple of 4 in 4 .. 128):
  gru_fwd_kernel<8, GRU>  / gru_bwd_kernel<8, GRU>    hidden <= 32       H = 4 (the floor), 20 (a partial second wavefront), 32
  gru_fwd_kernel<16, GRU> / gru_bwd_kernel<16, GRU>   32 < hidden <= 64  H = 36, 64
  gru_fwd_kernel<32, GRU> / gru_bwd_kernel<32, GRU>   64 < hidden        H = 68, 100, 128
  each at B = 1, 16 (a full tile), 17 (a tile holding one sample), 37 and L = 1, 2, 7 (both halves of the double-buffered
  state image); L = 200 at H = 64, B = 37 (the longest recurrence: the bar follows it through e32).
  Operands present or NULL: b_ih / b_hh, h0, lengths; d_out only, d_hn only (the other NULL in rbx_gru_bwd).
  lengths as int32 and int64; lengths of -3 and L + 5 (gru_lengths clamps to [0, L]; the restatement's ``lengths > t``).
  Through the C ABI: gi and d_out as views inside wider blocks (gi_stride_t = 3H + 4, gi_stride_b > L gi_stride_t; d_out
  likewise) whose filler is 1e30, the same bits as the contiguous call; the refusals of strides that are no multiple of 4
  floats and of gi_stride_t < 3H (status codes, nothing is launched); the saved tensor [B, L, 5, H] (r, z, n, gh_n, h_prev).
A spy on ops.lib counts rbx_gru_fwd / rbx_gru_bwd: the kernels ran, not the step-loop composition.

Measured on the MI355X, worst err / bar over all cases of this module (bar factor 4 everywhere):
  through ops.gru   out 0.12, h_n 0.15, dx 0.26, dW_ih 0.22, dW_hh 0.32, db_ih 0.15, db_hh 0.18, dh0 0.13
  through the C ABI out 0.06, h_n 0.05, saved 0.09, d_gi 0.16, dh0 0.09, the sum of d_gh_n (db_hh of the n gate) 0.14
  L = 200 is no worse than L = 7 (dx 0.14, dW_hh 0.13): the bar holds 3 to 20 times over."""
import ctypes

import pytest
import torch

from fp32_bar import assert_bar, report
from test_gpu_gru import _fused, _inputs, _names, _restatement, _run

pytestmark = pytest.mark.gpu
WIDTHS = [4, 20, 32, 36, 64, 68, 100, 128]
I = 12


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _spy(monkeypatch):
    from recbox_amd import ops
    calls = []
    real = ops.lib

    class Spy(object):
        def rbx_gru_fwd(self, *a):
            calls.append("fwd")
            return real.rbx_gru_fwd(*a)

        def rbx_gru_bwd(self, *a):
            calls.append("bwd")
            return real.rbx_gru_bwd(*a)

        def __getattr__(self, name):
            return getattr(real, name)
    monkeypatch.setattr(ops, "lib", Spy())
    return calls


def _check(inp, tag, **form):
    """ops.gru on the GPU against float64, the bar from the float32 CPU run of the same restatement."""
    want = _run(_restatement, inp, "cpu", torch.float64, **form)
    ref32 = _run(_restatement, inp, "cpu", torch.float32, **form)
    got = _run(_fused, inp, "cuda", torch.float32, **form)
    for what, a, b, c in zip(_names(1), got, want, ref32):
        assert (a is None) == (b is None), "%s %s" % (what, tag)
        if b is not None:
            assert_bar("%s %s" % (what.replace("_l0", ""), tag), a, b, c)


@pytest.mark.parametrize("H", WIDTHS)
def test_every_width_batch_and_length(H, monkeypatch):
    calls = _spy(monkeypatch)
    n = 0
    for B in (1, 16, 17, 37):
        for L in (1, 2, 7):
            _check(_inputs(B, L, I, H, seed=20), "H=%d B=%d L=%d" % (H, B, L))
            n += 1
    assert calls == ["fwd", "bwd"] * n
    report("gru widths H=%d" % H)


def test_longest_recurrence(monkeypatch):
    calls = _spy(monkeypatch)
    _check(_inputs(37, 200, I, 64, seed=21), "H=64 B=37 L=200")
    assert calls == ["fwd", "bwd"]
    report("gru L=200")


@pytest.mark.parametrize("use", [("out", "h_n"), ("out",), ("h_n",)], ids=["both", "d_out", "d_hn"])
@pytest.mark.parametrize("H", [20, 68])
def test_operands_present_or_null(H, use, monkeypatch):
    calls = _spy(monkeypatch)
    n = 0
    for bias in (True, False):
        for h0 in (True, False):
            for lengths in (True, False):
                _check(_inputs(17, 7, I, H, seed=22), "H=%d bias=%d h0=%d lengths=%d use=%s" % (H, bias, h0, lengths, "+".join(use)),
                       bias=bias, h0=h0, lengths=lengths, use=use)
                n += 1
    assert calls == ["fwd", "bwd"] * n
    report("gru operands H=%d %s" % (H, "+".join(use)))


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("H", [20, 36, 100])
def test_lengths_dtypes_and_clamp(H, dtype, monkeypatch):
    calls = _spy(monkeypatch)
    B, L = 37, 7
    inp = _inputs(B, L, I, H, seed=23)
    lengths = inp["lengths"].clone()
    lengths[0], lengths[1], lengths[2], lengths[3] = -3, L + 5, 0, L
    lengths[16], lengths[17], lengths[36] = L + 5, -3, L + 5          # both sides of a tile boundary, the last tile's only sample
    inp["lengths"] = lengths.to(dtype)
    _check(inp, "H=%d clamp %s" % (H, dtype))
    clamped = dict(inp)
    clamped["lengths"] = lengths.clamp(0, L).to(dtype)
    a = _run(_fused, inp, "cuda", torch.float32)
    b = _run(_fused, clamped, "cuda", torch.float32)
    for what, x, y in zip(_names(1), a, b):
        assert torch.equal(x, y), what
    assert calls == ["fwd", "bwd"] * 3
    report("gru lengths H=%d" % H)


# ---- the C entry points: strided gi / d_out, refusals, the saved tensor ----------------------------------------------------
def _cabi_case(B, L, H, seed):
    """The recurrence alone: gi is the input (w_ih = identity in the restatement, so gi = x exactly)."""
    g = torch.Generator().manual_seed(7000 + 100 * H + 10 * L + B + seed)
    bound = 1.0 / H ** 0.5
    uni = lambda *s: (torch.rand(*s, generator=g) * 2 - 1) * bound
    lengths = torch.randint(0, L + 1, (B,), generator=g)
    if B > 2:
        lengths[0], lengths[1], lengths[2] = L, 0, 1
    return {"gi": torch.randn(B, L, 3 * H, generator=g), "w_hh": uni(3 * H, H), "b_hh": uni(3 * H),
            "h0": torch.randn(B, H, generator=g), "lengths": lengths,
            "d_out": torch.randn(B, L, H, generator=g) / (B * L) ** 0.5, "d_hn": torch.randn(B, H, generator=g) / (B * L) ** 0.5}


def _cabi_reference(case, dtype):
    """out, h_n, saved [B, L, 5, H], d_gi, d_h0, db_hh of the n gate (= sum of d_gh_n) from tests/gru64.py; the saved gates
    are the restatement's formulas at h_prev = the state before the step."""
    import gru64
    gi, w_hh, b_hh, h0 = (case[n].to(dtype).requires_grad_(True) for n in ("gi", "w_hh", "b_hh", "h0"))
    H = w_hh.shape[1]
    out, hn = gru64.gru_layer(gi, torch.eye(3 * H, dtype=dtype), w_hh, None, b_hh, h0, case["lengths"])
    dgi, db, dh0 = torch.autograd.grad((out * case["d_out"].to(dtype)).sum() + (hn * case["d_hn"].to(dtype)).sum(), (gi, b_hh, h0))
    with torch.no_grad():
        hs, h = [], h0
        for t in range(gi.shape[1]):
            hs.append(h)
            h = torch.where((case["lengths"] > t).unsqueeze(1), out[:, t], h)
        hp = torch.stack(hs, dim=1)                                            # [B, L, H]
        gh = hp @ w_hh.t() + b_hh
        r = torch.sigmoid(gi[..., :H] + gh[..., :H])
        z = torch.sigmoid(gi[..., H:2 * H] + gh[..., H:2 * H])
        n = torch.tanh(gi[..., 2 * H:] + r * gh[..., 2 * H:])
        saved = torch.stack([r, z, n, gh[..., 2 * H:], hp], dim=2)
    return {"out": out.detach(), "h_n": hn.detach(), "saved": saved, "d_gi": dgi, "dh0": dh0, "db_hh_n": db[2 * H:]}


def _wide(t, pad_t, pad_b, filler=1e30):
    """``t`` [B, L, W] as a view inside a wider block: row stride W + pad_t, sample stride L (W + pad_t) + pad_b."""
    B, L, W = t.shape
    block = torch.full((B, L * (W + pad_t) + pad_b), filler, device=t.device)
    view = block.as_strided((B, L, W), (L * (W + pad_t) + pad_b, W + pad_t, 1))
    view.copy_(t)
    return block, view


def _cabi_run(case, gi, d_out, lengths_dtype=torch.int64):
    """rbx_gru_fwd + rbx_gru_bwd on device tensors ``gi`` / ``d_out`` (any strides the entry points accept)."""
    from recbox_amd import _lib
    lib = _lib.lib
    B, L, H3 = gi.shape
    H = H3 // 3
    dev = gi.device
    w_hh, b_hh, h0, d_hn = (case[n].to(dev) for n in ("w_hh", "b_hh", "h0", "d_hn"))
    lengths = case["lengths"].to(dev).to(lengths_dtype)
    code = _lib.RBX_I32 if lengths_dtype == torch.int32 else _lib.RBX_I64
    nan = lambda *s: torch.full(s, float("nan"), device=dev)
    out, saved, hn = nan(B, L, H), nan(B, L, 5, H), nan(B, H)
    rc = lib.rbx_gru_fwd(_p(gi), gi.stride(0), gi.stride(1), _p(w_hh), _p(b_hh), _p(h0), _p(lengths), code, B, L, H,
                         _lib.RBX_F32, _p(out), _p(saved), _p(hn), None)
    assert rc == 0, _lib.last_error()
    dgi, dghn, dh0 = nan(B, L, 3 * H), nan(B, L, H), nan(B, H)
    rc = lib.rbx_gru_bwd(_p(saved), _p(w_hh), _p(d_out), d_out.stride(0), d_out.stride(1), _p(d_hn), _p(lengths), code, B, L, H,
                         _lib.RBX_F32, _p(dgi), _p(dghn), _p(dh0), None)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    return {"out": out, "h_n": hn, "saved": saved, "d_gi": dgi, "dh0": dh0, "d_gh_n": dghn}


@pytest.mark.parametrize("B,L,H", [(17, 7, 4), (37, 2, 20), (17, 7, 36), (37, 7, 64), (17, 2, 68), (37, 7, 100), (17, 1, 128)])
def test_c_abi_strided_operands_and_saved_tensor(B, L, H):
    case = _cabi_case(B, L, H, seed=24)
    want, ref32 = _cabi_reference(case, torch.float64), _cabi_reference(case, torch.float32)
    gi, d_out = case["gi"].cuda(), case["d_out"].cuda()
    plain = _cabi_run(case, gi, d_out)
    gi_block, gi_view = _wide(gi, 4, 8)
    do_block, do_view = _wide(d_out, 4, 8)
    assert gi_view.stride(1) == 3 * H + 4 and gi_view.stride(0) > L * gi_view.stride(1) and not gi_view.is_contiguous()
    assert do_view.stride(1) == H + 4 and do_view.stride(0) > L * do_view.stride(1)
    strided = _cabi_run(case, gi_view, do_view, torch.int32)
    for name in plain:                                                          # a kernel that ignores a stride reads 1e30
        assert torch.equal(plain[name], strided[name]), name
    assert (gi_block.as_strided((B, L, 4), (gi_view.stride(0), gi_view.stride(1), 1), 3 * H) == 1e30).all()
    tag = "B=%d L=%d H=%d" % (B, L, H)
    live = (torch.arange(L).unsqueeze(0) < case["lengths"].unsqueeze(1))        # the saved rows the backward reads
    for name in ("out", "h_n", "d_gi", "dh0"):
        assert_bar("%s c-abi %s" % (name, tag), strided[name], want[name], ref32[name])
    assert_bar("saved c-abi " + tag, strided["saved"].cpu()[live], want["saved"][live], ref32["saved"][live])
    assert_bar("db_hh_n c-abi " + tag, strided["d_gh_n"].double().sum((0, 1)), want["db_hh_n"], ref32["db_hh_n"])
    dead = ~live
    assert (strided["out"].cpu()[dead] == 0).all() and (strided["d_gi"].cpu()[dead] == 0).all()
    assert (strided["d_gh_n"].cpu()[dead] == 0).all()
    report("gru c-abi " + tag)


def test_c_abi_refuses_strides_it_cannot_read():
    """Status codes only: a refused call launches nothing (the outputs keep their NaN fill)."""
    from recbox_amd import _lib
    lib = _lib.lib
    B, L, H = 5, 3, 8
    case = _cabi_case(B, L, H, seed=25)
    w_hh, b_hh, h0, d_hn = (case[n].cuda() for n in ("w_hh", "b_hh", "h0", "d_hn"))
    gi = torch.zeros(B, L * (3 * H + 8) + 8, device="cuda")
    d_out = torch.zeros(B, L * (H + 8) + 8, device="cuda")
    nan = lambda *s: torch.full(s, float("nan"), device="cuda")
    out, saved, hn = nan(B, L, H), nan(B, L, 5, H), nan(B, H)

    def fwd(stride_b, stride_t, base=gi):
        return lib.rbx_gru_fwd(_p(base), stride_b, stride_t, _p(w_hh), _p(b_hh), _p(h0), None, 0, B, L, H, _lib.RBX_F32,
                               _p(out), _p(saved), _p(hn), None)
    assert fwd(L * 3 * H, 3 * H + 2) == _lib.RBX_ERR_UNSUPPORTED              # a row stride that is no multiple of 4 floats
    assert fwd(L * (3 * H + 4) + 2, 3 * H + 4) == _lib.RBX_ERR_UNSUPPORTED    # a sample stride that is none
    assert fwd(L * 3 * H, 3 * H - 4) == _lib.RBX_ERR_UNSUPPORTED              # rows that overlap: gi_stride_t < 3H
    assert fwd(L * 3 * H, 3 * H, gi.reshape(-1)[1:]) == _lib.RBX_ERR_UNSUPPORTED      # a base that is not 16-byte aligned
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(saved).all() and torch.isnan(hn).all()
    assert fwd(L * (3 * H + 4) + 8, 3 * H + 4) == _lib.RBX_OK
    dgi, dghn, dh0 = nan(B, L, 3 * H), nan(B, L, H), nan(B, H)

    def bwd(stride_b, stride_t, base=d_out):
        return lib.rbx_gru_bwd(_p(saved), _p(w_hh), _p(base), stride_b, stride_t, _p(d_hn), None, 0, B, L, H, _lib.RBX_F32,
                               _p(dgi), _p(dghn), _p(dh0), None)
    assert bwd(L * H, H + 2) == _lib.RBX_ERR_UNSUPPORTED
    assert bwd(L * (H + 4) + 2, H + 4) == _lib.RBX_ERR_UNSUPPORTED
    assert bwd(L * H, H - 4) == _lib.RBX_ERR_UNSUPPORTED
    assert bwd(L * H, H, d_out.reshape(-1)[1:]) == _lib.RBX_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.isnan(dgi).all() and torch.isnan(dghn).all() and torch.isnan(dh0).all()
    assert bwd(L * (H + 4) + 8, H + 4) == _lib.RBX_OK
    torch.cuda.synchronize()
    assert not torch.isnan(dgi).any() and not torch.isnan(dh0).any()
