"""The fused additive attention pooling on the HIP path (csrc/rbx_addattn.hip: ops.additive_attn_pool, the NARM and STAMP
mirrors) against the float64 restatement of tests/addattn64.py on the CPU, within the project's absolute 1e-4 (the fp32
composition is within 1e-6 of that restatement with these draws: addattn64's docstring).  Inputs: addattn64.make_case."""
import functools

import pytest
import torch

import addattn64
from conftest import Fixture, assert_close, assert_grads_close

pytestmark = pytest.mark.gpu
TOL = 1e-4
# (L, D, H): one position at the floor; one tile, one wavefront; L off the tile, D != H, neither a multiple of 16; four
# wavefronts over four tiles; NARM's default (seven wavefronts, the last a quarter full); the top class over 13 tiles
SHAPES = [(1, 4, 4), (7, 16, 16), (17, 20, 12), (50, 64, 64), (20, 100, 100), (200, 128, 128)]
BATCHES = [1, 37]


@functools.lru_cache(maxsize=None)
def _case(B, L, D, H, seed=0):
    return addattn64.make_case(B, L, D, H, seed)


@functools.lru_cache(maxsize=None)
def _ref(B, L, D, H, seed=0, use_ctx=True, masked=True, eps=0.0):
    return addattn64.reference(_case(B, L, D, H, seed), use_ctx=use_ctx, masked=masked, eps=eps)


def _fused(*a):
    from recbox_amd import ops
    return ops.additive_attn_pool(*a)


def _composition(*a):
    from recbox_amd import ops
    return ops.additive_attn_pool_torch(*a)


def _check(got, ref, what):
    for n in addattn64.NAMES:
        if ref[n] is None:
            assert got[n] is None, n
        else:
            assert_close(got[n], ref[n], TOL, "%s %s" % (what, n))


def _same_bits(a, b, what=""):
    for n in addattn64.NAMES:
        if a[n] is None:
            assert b[n] is None
        else:
            assert torch.equal(a[n], b[n]), "%s %s" % (what, n)


def _spy(monkeypatch):
    """Counts the calls that reach rbx_addattn_fwd."""
    from recbox_amd import ops
    calls = []
    fwd = ops.lib.rbx_addattn_fwd

    class Spy(object):
        def rbx_addattn_fwd(self, *a):
            calls.append("fwd")
            return fwd(*a)

        def __getattr__(self, name):
            return getattr(ops._lib.lib, name)
    monkeypatch.setattr(ops, "lib", Spy())
    return calls


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("L,D,H", SHAPES)
def test_against_float64(L, D, H, B, monkeypatch):
    from recbox_amd import ops
    assert ops.additive_attn_supported(D, H, L)
    calls = _spy(monkeypatch)
    what = "B=%d L=%d D=%d H=%d" % (B, L, D, H)
    _check(addattn64.run(_fused, _case(B, L, D, H), "cuda"), _ref(B, L, D, H), what)
    assert calls == ["fwd"]                                   # the kernels ran, not the composition
    _check(addattn64.run(_composition, _case(B, L, D, H), "cuda"), _ref(B, L, D, H), what + " composition")


@pytest.mark.parametrize("L,D,H", [(7, 16, 16), (17, 20, 12), (20, 100, 100)])
def test_forms(L, D, H):
    """Without ctx; without mask; with neither; with eps > 0."""
    B = 37
    case = _case(B, L, D, H, 1)
    for use_ctx, masked in ((False, True), (True, False), (False, False)):
        got = addattn64.run(_fused, case, "cuda", use_ctx=use_ctx, masked=masked)
        _check(got, _ref(B, L, D, H, 1, use_ctx, masked), "ctx=%s mask=%s" % (use_ctx, masked))
    _check(addattn64.run(_fused, case, "cuda", eps=1e-12), _ref(B, L, D, H, 1, True, True, 1e-12), "eps=1e-12")


@pytest.mark.parametrize("L,D,H", [(17, 20, 12), (50, 64, 64)])
def test_mask_dtypes_and_eps_give_the_same_bits(L, D, H):
    case = _case(37, L, D, H, 2)
    base = addattn64.run(_fused, case, "cuda")
    m = case["mask"].cuda()
    for mask in (m.bool(), m.int(), m.float(), m.to(torch.uint8)):
        _same_bits(addattn64.run(_fused, case, "cuda", mask=mask), base, str(mask.dtype))
    _same_bits(addattn64.run(_fused, case, "cuda", eps=1e-12), base, "eps")     # every row has a valid position


@pytest.mark.parametrize("L,D,H", [(17, 20, 12), (50, 64, 64)])
def test_strided_view_of_a_wider_block(L, D, H, monkeypatch):
    calls = _spy(monkeypatch)
    case = _case(37, L, D, H, 3)
    wide = torch.zeros(37, L + 3, D + 12, device="cuda")
    wide[:, 1:L + 1, 8:8 + D] = case["x"].cuda()
    wide.requires_grad_(True)
    view = wide[:, 1:L + 1, 8:8 + D]
    assert not view.is_contiguous() and view.data_ptr() % 16 == 0
    x, w, c, v = view, *(case[n].cuda().requires_grad_(True) for n in ("w", "ctx", "v"))
    out, alpha = _fused(x, w, c, v, case["mask"].cuda(), 0.0)
    (out * case["g_out"].cuda()).sum().backward()
    assert calls == ["fwd"]
    ref = _ref(37, L, D, H, 3)
    got = {"out": out, "alpha": alpha, "dx": wide.grad[:, 1:L + 1, 8:8 + D], "dw": w.grad, "dctx": c.grad, "dv": v.grad}
    _check(got, ref, "strided view")
    rest = wide.grad.clone()
    rest[:, 1:L + 1, 8:8 + D] = 0
    assert (rest == 0).all()


def test_one_valid_position_gives_alpha_one_and_that_row():
    B, L, D, H = 37, 17, 20, 12
    case = _case(B, L, D, H, 4)
    pos = torch.arange(B) % L
    mask = torch.zeros(B, L, dtype=torch.long)
    mask[torch.arange(B), pos] = 1
    for eps in (0.0, 1e-12):
        got = addattn64.run(_fused, case, "cuda", mask=mask.cuda(), eps=eps)
        assert torch.equal(got["alpha"].cpu(), mask.float())                    # exactly 1.0 and exactly 0.0
        assert torch.equal(got["out"].cpu(), case["x"][torch.arange(B), pos])
        assert (got["dx"].cpu()[mask == 0] == 0).all()


@pytest.mark.parametrize("k", [3, 7])
def test_equal_logits_give_exactly_one_over_k(k):
    B, L, D, H = 37, 17, 20, 12
    case = dict(_case(B, L, D, H, 5))
    case["v"] = torch.zeros(H)
    mask = torch.zeros(B, L, dtype=torch.long)
    for b in range(B):
        mask[b, torch.randperm(L, generator=torch.Generator().manual_seed(b))[:k]] = 1
    got = addattn64.run(_fused, case, "cuda", mask=mask.cuda())
    expect = (torch.tensor(1.0) / torch.tensor(float(k))).item()                # what 1.0f / k rounds to
    assert torch.equal(got["alpha"].cpu(), mask.float() * expect)


def test_masked_positions_are_exactly_zero():
    B, L, D, H = 37, 50, 64, 64
    case = _case(B, L, D, H, 6)
    got = addattn64.run(_fused, case, "cuda")
    dead = (case["mask"] == 0).cuda()
    assert dead.any() and (~dead).any()
    assert (got["alpha"][dead] == 0).all() and (got["dx"][dead] == 0).all()
    assert (got["alpha"][~dead] > 0).all() and (got["dx"][~dead] != 0).any()


def test_all_masked_row():
    """eps > 0: zeros, and no gradient leaves the row; eps = 0: NaN, as the composition's plain division."""
    B, L, D, H = 37, 7, 16, 16
    case = _case(B, L, D, H, 7)
    mask = case["mask"].clone()
    mask[5] = 0
    got = addattn64.run(_fused, case, "cuda", mask=mask.cuda(), eps=1e-12)
    assert (got["alpha"][5] == 0).all() and (got["out"][5] == 0).all() and (got["dx"][5] == 0).all()
    assert (got["dctx"][5] == 0).all()
    comp = addattn64.run(_composition, case, "cuda", mask=mask.cuda(), eps=1e-12)
    for n in addattn64.NAMES:
        assert_close(got[n], comp[n], TOL, "all-masked row " + n)
    got = addattn64.run(_fused, case, "cuda", mask=mask.cuda(), eps=0.0)
    assert torch.isnan(got["alpha"][5]).all() and torch.isnan(got["out"][5]).all()
    keep = torch.arange(B) != 5
    assert_close(got["out"][keep], _ref(B, L, D, H, 7)["out"][keep], TOL, "the other rows")


@pytest.mark.parametrize("L,D,H", [(50, 64, 64), (20, 100, 100), (200, 128, 128)])
def test_determinism(L, D, H):
    case = _case(37, L, D, H, 8)
    _same_bits(addattn64.run(_fused, case, "cuda"), addattn64.run(_fused, case, "cuda"))


def test_nothing_of_B_L_H_is_saved():
    B, L, D, H = 37, 50, 64, 64
    case = _case(B, L, D, H, 9)
    bound = B * L * D + B * L + B * (D + H) + H * D + H + B * L

    def saved(fn):
        seen = []
        x, w, c, v = (case[n].cuda().requires_grad_(True) for n in ("x", "w", "ctx", "v"))
        with torch.autograd.graph.saved_tensors_hooks(lambda t: seen.append(t.numel()) or t, lambda t: t):
            out, _ = fn(x, w, c, v, case["mask"].cuda(), 0.0)
        out.sum().backward()
        return sum(seen)
    assert saved(_fused) < bound
    assert saved(_composition) > bound                        # the counter sees the [B, L, H] layers the composition keeps


def test_switch_and_refusals_agree_with_the_kernel(monkeypatch):
    from recbox_amd import ops
    calls = _spy(monkeypatch)
    B, L, D, H = 37, 17, 20, 12
    case = _case(B, L, D, H, 10)
    fused = addattn64.run(_fused, case, "cuda")
    assert calls == ["fwd"]
    monkeypatch.setattr(ops.config, "addattn_fused", False)
    off = addattn64.run(_fused, case, "cuda")
    monkeypatch.setattr(ops.config, "addattn_fused", True)
    assert calls == ["fwd"]
    for n in addattn64.NAMES:
        assert_close(off[n], fused[n], TOL, "switch off " + n)
    assert not ops.additive_attn_supported(6, 12, L)
    small = _case(B, L, 6, 12, 10)                            # D = 6: refused, the composition under the same entry point
    _check(addattn64.run(_fused, small, "cuda"), _ref(B, L, 6, 12, 10), "refused D=6")
    odd = torch.randn(B, L, D + 1, device="cuda")[:, :, 1:]   # rows neither aligned nor a multiple of 4 apart
    ops.additive_attn_pool(odd, case["w"].cuda(), None, case["v"].cuda())
    ops.additive_attn_pool(case["x"].cuda().double(), case["w"].cuda().double(), None, case["v"].cuda().double())
    out, alpha = ops.additive_attn_pool(torch.zeros(0, L, D, device="cuda"), case["w"].cuda(), None, case["v"].cuda())
    assert tuple(out.shape) == (0, D) and tuple(alpha.shape) == (0, L)
    assert calls == ["fwd"]


# ---- models -----------------------------------------------------------------------------------------------------------------
def _mirror():
    from test_addattn_host import _mirror as build
    return build()


def _stamp_step(model, ids):
    z = model({"session": ids})
    z.sum().backward()
    return z


def test_stamp_matches_the_reference_fixture(monkeypatch):
    calls = _spy(monkeypatch)
    fx = Fixture("rechub_stamp")
    model = _mirror()
    model.load_state_dict(fx.tensors("p_stamp"), strict=True)
    model = model.cuda().train()
    z = _stamp_step(model, fx.tensors("in", device="cuda")["session"])
    assert calls == ["fwd"]
    assert_close(z, fx["out_stamp"]["z"], TOL, "z")
    assert_grads_close(model, fx["g_stamp"], TOL)


def test_stamp_does_not_fault_on_an_empty_session():
    fx = Fixture("rechub_stamp")
    model = _mirror()
    model.load_state_dict(fx.tensors("p_stamp"), strict=True)
    model = model.cuda().train()
    ids = fx.tensors("in", device="cuda")["session"].clone()
    ids[3] = 0
    z = _stamp_step(model, ids)
    torch.cuda.synchronize()
    keep = torch.arange(ids.shape[0]) != 3
    assert_close(z[keep], fx["out_stamp"]["z"][keep.numpy()], TOL, "the other sessions")


def test_stamp_step_is_capturable_and_replays_the_eager_bits(monkeypatch):
    from recbox_amd import ops
    from test_gpu_gru import _capture
    monkeypatch.setattr(ops.config, "check_ids", False)      # the id check of the lookup reads a status word on the host
    fx = Fixture("rechub_stamp")
    ids = fx.tensors("in", device="cuda")["session"]

    def make():
        m = _mirror()
        m.load_state_dict(fx.tensors("p_stamp"), strict=True)
        return m.cuda().train()
    eager = make()
    z_e = _stamp_step(eager, ids)
    model = make()
    buf = torch.ones_like(ids)

    def zero():
        for p in model.parameters():
            p.grad = None
    graph, z = _capture(lambda: _stamp_step(model, buf), zero)
    buf.copy_(ids)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(z.detach(), z_e.detach())
    for (n, a), (_, b) in zip(model.named_parameters(), eager.named_parameters()):
        assert torch.equal(a.grad, b.grad), n
