"""oracle/interact64.py on the CPU: every restatement equals float64 autograd of the naive torch expression, modes 0-3
reproduce the live reference's fixtures, the float32 sequential C restatement (oracle/liborc.so) stays inside the bound
(the proof that a correct float32 implementation can meet it), and the bound catches one lost term: a field, the last
live lane's element, a pair, a history step.  The input builders are shared with tests/test_gpu_interact_dims.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F_

from conftest import Fixture
from oracle import interact64 as I

EPS32 = I.EPS32


# ---- inputs ---------------------------------------------------------------------------------------------------------
def randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def one_signed(shape, seed):
    """Positive, same magnitude (0.5 .. 1.5): where a biased or mis-ordered sum, or a lost term, cannot hide."""
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed)) + 0.5


def spread(shape, seed):
    """Mixed sign, magnitudes spread over e^-6 .. e^+6."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * torch.exp(12.0 * torch.rand(shape, generator=g) - 6.0)


KINDS = {"randn": randn, "one_signed": one_signed, "spread": spread}


def value_safe(e):
    """Rows with |sum_d e| < 1e-3 sum_d |e| get one entry replaced by the row's abs sum: denom 1's count is no knife edge."""
    e = e.clone()
    s, a = e.double().sum(-1).abs(), e.double().abs().sum(-1)
    bad = (a != 0) & (s < 2e-3 * a)
    e[..., 0] = torch.where(bad, a.float(), e[..., 0])
    I.assert_value_rows_are_safe(e)
    return e


def _rel(a, b):
    return float((a - b).abs().max() / (b.abs().max() + 1e-300)) if b.numel() else 0.0


# ---- the restatements equal float64 autograd of the naive expressions -------------------------------------------------
def _naive_modes(e):
    F = e.shape[1]
    S, Q = e.sum(1), (e * e).sum(1)
    bi = 0.5 * (S * S - Q)
    ip = torch.bmm(e, e.transpose(1, 2))
    mask = torch.triu(torch.ones(F, F), 1).bool()
    idx = torch.triu_indices(F, F, offset=1)
    return {"bi": bi, "ps": bi.sum(1, keepdim=True), "ip": ip[:, mask], "ew": e[:, idx[0]] * e[:, idx[1]]}


@pytest.mark.parametrize("F,D", [(1, 3), (2, 1), (6, 8), (39, 16), (7, 33)])
def test_modes_equal_float64_autograd(F, D):
    e = randn((5, F, D), F * 100 + D).double().requires_grad_(True)
    naive = _naive_modes(e)
    for key, fwd, grad in (("bi", I.bi_interaction64, I.fm_grad64), ("ps", I.product_sum64, I.fm_grad64),
                           ("ip", I.inner_product64, I.pair_grad64), ("ew", I.elementwise_product64, I.pair_grad64)):
        g = randn(naive[key].shape, 7 + D)
        want, A = fwd(e)
        tol = 1e-12 if key != "ew" else 1e-6                      # mode 3's want is the float32 product
        assert _rel(want, naive[key].detach()) <= tol, key
        assert bool((A >= want.abs() * (1 - 1e-12)).all()), key
        (de,) = torch.autograd.grad(naive[key], e, g.double(), retain_graph=True)
        gw, gA = grad(e, g)
        assert _rel(gw, de) <= 1e-12, key
        assert bool((gA >= gw.abs() * (1 - 1e-12)).all()), key
        if F == 1 and key in ("ip", "ew"):
            assert want.numel() == 0 and int(torch.count_nonzero(gw)) == 0 and int(torch.count_nonzero(gA)) == 0


def test_fm_sum_equals_float64_autograd():
    F, D, B = 5, 12, 9
    x = randn((B, F * D + 3), 1).double()
    w, b = randn((1, F * D), 2).double(), randn((1,), 3).double()
    out = I.fm_sum64(x, F, D, w, b)
    e = x[:, :F * D].view(B, F, D)
    assert _rel(out["S"][0], e.sum(1)) <= 1e-12
    assert _rel(out["y_fm"][0], _naive_modes(e)["ps"]) <= 1e-12
    assert _rel(out["y_lr"][0], F_.linear(x[:, :F * D], w, b)) <= 1e-12


@pytest.mark.parametrize("per_pair", [False, True])
@pytest.mark.parametrize("F,D", [(1, 4), (2, 1), (5, 4), (9, 7)])
def test_pair_mul_equals_float64_autograd(F, D, per_pair):
    B, P = 4, F * (F - 1) // 2
    right = randn((B, F, D), 1).double().requires_grad_(True)
    left = randn((B, P if per_pair else F, D), 2).double().requires_grad_(True)
    idx = torch.triu_indices(F, F, offset=1)
    out = (left if per_pair else left[:, idx[0]]) * right[:, idx[1]]
    g = randn((B, P, D), 3)
    want, _ = I.pair_mul64(left, right, per_pair)
    assert _rel(want, out.detach()) <= 1e-6
    (dl, al), (dr, ar) = I.pair_mul_grad64(left, right, g, per_pair)
    if P:
        rl, rr = torch.autograd.grad(out, (left, right), g.double())
        assert _rel(dl, rl) <= (1e-6 if per_pair else 1e-12) and _rel(dr, rr) <= 1e-12
    else:
        assert int(torch.count_nonzero(dl)) == 0 and int(torch.count_nonzero(dr)) == 0
        assert int(torch.count_nonzero(al)) == 0 and int(torch.count_nonzero(ar)) == 0


@pytest.mark.parametrize("D", [1, 7, 64, 200])
def test_l2_normalize_and_pair_dot_equal_float64_autograd(D):
    x = randn((6, 3, D), D).double()
    x[1, 1] = 0
    x[2, 0] *= 1e-14                                          # below eps: the clamped branch
    x = x.float().double().requires_grad_(True)
    dy = randn((6, 3, D), D + 1)
    y, _, clamped = I.l2_normalize64(x)
    ref = F_.normalize(x, p=2, dim=-1, eps=float(torch.tensor(1e-12, dtype=torch.float32)))
    assert _rel(y, ref.detach()) <= 1e-12
    assert clamped[1, 1] and clamped[2, 0] and int(clamped.sum()) == 2
    (dx,) = torch.autograd.grad(ref, x, dy.double())
    want, A = I.l2_normalize_grad64(x, dy)
    live = ~clamped
    assert float((want[live] - dx[live]).abs().max()) <= 1e-12 * float(A[live].max())   # D = 1: the two terms cancel to zero
    # clamped rows: the kernel's rule is plain dy / eps (torch's clamp_min passes no gradient through the norm either)
    assert _rel(want[clamped], dx[clamped]) <= 1e-12
    assert bool((A >= want.abs() * (1 - 1e-12)).all())
    u = randn((6, 1, D), 5).double().requires_grad_(True)
    v = randn((6, 4, D), 6).double().requires_grad_(True)
    g = randn((6, 4), 7)
    out = 0.25 * torch.einsum("bd,bnd->bn", u[:, 0], v)
    want, _ = I.pair_dot64(u, v, 0.25)
    assert _rel(want, out.detach()) <= 1e-12
    ru, rv = torch.autograd.grad(out, (u, v), g.double())
    (du, _), (dv, _) = I.pair_dot_grad64(u, v, g, 0.25)
    assert du.shape == u.shape and dv.shape == v.shape
    assert _rel(du, ru) <= 1e-12 and _rel(dv, rv) <= 1e-12


@pytest.mark.parametrize("numer_masked", [False, True])
@pytest.mark.parametrize("denom", [0, 1, 2, 3])
def test_pool_equals_float64_autograd(denom, numer_masked):
    B, L, D = 7, 6, 5
    e = value_safe(randn((B, L, D), denom)).double()
    e[2] = 0
    e[3, 4:] = 0
    mask = (torch.rand(B, L, generator=torch.Generator().manual_seed(9)) < 0.6).double()
    mask[5] = 0
    e.requires_grad_(True)
    eps = float(torch.tensor(1e-12, dtype=torch.float32))
    numer = (mask[:, :, None] * e).sum(1) if numer_masked else e.sum(1)
    den = {0: None, 1: (e.detach().sum(2) != 0).double().sum(1), 2: mask.sum(1), 3: torch.full((B,), float(L)).double()}[denom]
    out = numer if den is None else numer / (den + eps)[:, None]
    want, A = I.pool64(e, mask, numer_masked, denom, 1e-12)
    assert _rel(want, out.detach()) <= 1e-12
    dout = randn((B, D), 11)
    (de,) = torch.autograd.grad(out, e, dout.double())
    gw, gA = I.pool_grad64(e, dout, mask, numer_masked, denom, 1e-12)
    assert _rel(gw, de) <= 1e-12
    assert int(torch.count_nonzero(want[2])) == 0 and int(torch.count_nonzero(A[2])) == 0
    if numer_masked:
        assert int(torch.count_nonzero(gA[5])) == 0                 # masked steps: A = 0, exactly zero asked


# ---- anchors to the live reference's fixtures ---------------------------------------------------------------------------
def test_modes_reproduce_the_inner_product_fixture():
    fx = Fixture("inner_product")
    e = torch.from_numpy(fx["in"]["E"])
    for mode, fwd, grad, C in (("product_sum", I.product_sum64, I.fm_grad64, I.c_fm_fwd(6)),
                               ("bi_interaction", I.bi_interaction64, I.fm_grad64, I.c_fm_fwd(6)),
                               ("inner_product", I.inner_product64, I.pair_grad64, I.c_inner(8)),
                               ("elementwise_product", I.elementwise_product64, I.pair_grad64, 1),
                               ("rechub_fm_1", I.product_sum64, I.fm_grad64, I.c_fm_fwd(6)),
                               ("rechub_fm_0", I.bi_interaction64, I.fm_grad64, I.c_fm_fwd(6))):
        want, A = fwd(e)
        got = torch.from_numpy(fx["out"][mode])
        assert float(I.ratios(got, want, A, C).max()) <= 1.0, mode
        R = torch.from_numpy(fx["in"]["R_" + mode])                # the fixture's loss is sum(out * R)
        gw, gA = grad(e, R)
        gg = torch.from_numpy(fx["g"][mode])
        assert float(I.ratios(gg, gw, gA, I.C_BOUND).max()) <= 1.0, mode


def test_pair_mul_reproduces_the_bilinear_fixtures_pairing():
    fx = Fixture("bilinear")
    x = torch.from_numpy(fx["in"]["x"])
    for kind, per_pair in (("field_all", False), ("field_each", False), ("field_interaction", True)):
        ref = fx["out_" + kind + "_v2"]
        W = torch.from_numpy(ref["W"]).double()
        i, _ = I.pairs(x.shape[1])
        if kind == "field_all":
            left = x.double() @ W
        elif kind == "field_each":
            left = torch.einsum("bfd,fde->bfe", x.double(), W)
        else:
            left = torch.einsum("bpd,pde->bpe", x.double()[:, i], W)
        want, _ = I.pair_mul64(left, x, per_pair)
        y = torch.from_numpy(ref["y"]).double()
        assert float((want - y).abs().max()) <= 1e-5, kind


# ---- a correct float32 implementation meets the bound ----------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("D", [1, 16, 255, 1024])
@pytest.mark.parametrize("F", [2, 6, 39, 200])
def test_the_sequential_float32_restatement_is_inside_the_bound(F, D, kind):
    from oracle import c_oracle as C
    lib = C.load()
    B = 5
    e = KINDS[kind]((B, F, D), F * 7 + D)
    en = np.ascontiguousarray(e.numpy())
    P = F * (F - 1) // 2
    worst = {}
    for mode, fwd, shape, Cb in ((0, I.product_sum64, (B, 1), I.c_fm_fwd(F)), (1, I.bi_interaction64, (B, D), I.c_fm_fwd(F)),
                                 (2, I.inner_product64, (B, P), I.c_inner(D)), (3, I.elementwise_product64, (B, P, D), None)):
        if mode >= 2 and F > 39:
            continue
        out = np.zeros(shape, dtype=np.float32)
        lib.orc_interaction_fwd(C.ptr(en), B, F, D, mode, C.ptr(out))
        want, A = fwd(e)
        if Cb is None:
            assert torch.equal(torch.from_numpy(out).double(), want)
            continue
        worst[mode] = float(I.ratios(torch.from_numpy(out), want, A, Cb).max())
    rows = np.ascontiguousarray(e.reshape(B * F, D).numpy())
    y = np.zeros_like(rows)
    lib.orc_l2norm_fwd(C.ptr(rows), B * F, D, 1e-12, C.ptr(y))
    want, A, _ = I.l2_normalize64(torch.from_numpy(rows))
    worst["l2norm"] = float(I.ratios(torch.from_numpy(y), want, A, I.c_rows(D)).max())
    u = np.ascontiguousarray(KINDS[kind]((B, D), 3).numpy())
    out = np.zeros((B, F), dtype=np.float32)
    lib.orc_pairdot_fwd(C.ptr(u), C.ptr(en), B, F, D, 0.25, C.ptr(out))
    want, A = I.pair_dot64(torch.from_numpy(u), e, 0.25)
    worst["pairdot"] = float(I.ratios(torch.from_numpy(out), want, A, I.c_rows(D)).max())
    print("F%d D%d %s: %s" % (F, D, kind, ", ".join("%s %.3g" % kv for kv in worst.items())))
    assert max(worst.values()) <= 1.0, worst


# ---- the bar catches one lost term ------------------------------------------------------------------------------------------
def _only(r, hit, what):
    """Every element of ``hit`` exceeds the bound and no other element does."""
    assert bool(hit.any()), what
    assert float(r[hit].min()) > 1.0, "%s: a lost term stays inside the bound (%.3g)" % (what, float(r[hit].min()))
    assert float(r[~hit].max() if bool((~hit).any()) else 0.0) <= 1.0, what


def _orc_modes(e, mode):
    from oracle import c_oracle as C
    B, F, D = e.shape
    shape = {0: (B, 1), 1: (B, D), 2: (B, F * (F - 1) // 2)}[mode]
    out = np.zeros(shape, dtype=np.float32)
    C.load().orc_interaction_fwd(C.ptr(np.ascontiguousarray(e.numpy())), B, F, D, mode, C.ptr(out))
    return torch.from_numpy(out)


@pytest.mark.parametrize("F", [2, 39, 200])
def test_one_lost_field_in_one_sample_is_caught(F):
    """Float32 sequential results over the batch with field F - 1 of sample 3 left out (the tail of the row unroll)."""
    B, D = 6, 16
    e = one_signed((B, F, D), F)
    lost = e.clone()
    lost[3, F - 1] = 0
    for mode, fwd in ((0, I.product_sum64), (1, I.bi_interaction64)):
        want, A = fwd(e)
        hit = torch.zeros(want.shape, dtype=torch.bool)
        hit[3] = True
        _only(I.ratios(_orc_modes(lost, mode), want, A, I.c_fm_fwd(F)), hit, "mode %d F%d" % (mode, F))
    for g in (one_signed((B, 1), 5), one_signed((B, D), 6)):         # the gradient: S without the field
        want, A = I.fm_grad64(e, g)
        S = lost.double().sum(1, keepdim=True).float()
        got = g.view(B, 1, -1) * (S - e)
        hit = torch.zeros(want.shape, dtype=torch.bool)
        hit[3] = True
        _only(I.ratios(got, want, A, I.c_fm_bwd(F)), hit, "gradient F%d" % F)
    w, b = one_signed((1, F * D), 8), one_signed((1,), 9)            # fm_sum's S and the first-order sum
    parts = I.fm_sum64(e.reshape(B, F * D), F, D, w, b)
    hit = torch.zeros(B, D, dtype=torch.bool)
    hit[3] = True
    _only(I.ratios(lost.sum(1), *parts["S"], I.c_fm_fwd(F)), hit, "fm_sum S F%d" % F)
    got = F_.linear(lost.reshape(B, F * D), w, b)
    _only(I.ratios(got, *parts["y_lr"], I.c_fm_fwd(F)), hit[:, :1], "fm_sum y_lr F%d" % F)


def test_one_lost_element_of_the_last_live_lane_is_caught():
    """D = 132 = 33 float4 units in a 64-lane group: element d = D - 1 of sample 2 left out."""
    B, F, D = 5, 6, 132
    e = one_signed((B, F, D), 132)
    lost = e.clone()
    lost[2, :, D - 1] = 0
    want, A = I.product_sum64(e)
    hit = torch.zeros(B, 1, dtype=torch.bool)
    hit[2] = True
    _only(I.ratios(_orc_modes(lost, 0), want, A, I.c_fm_fwd(F)), hit, "product_sum")
    want, A = I.bi_interaction64(e)
    hit = torch.zeros(B, D, dtype=torch.bool)
    hit[2, D - 1] = True
    _only(I.ratios(_orc_modes(lost, 1), want, A, I.c_fm_fwd(F)), hit, "bi_interaction")
    x = e[:, 0]
    want, A, _ = I.l2_normalize64(x)
    got = F_.normalize(lost[:, 0], dim=-1)                         # the norm without the element: every d of the row moves
    hit = torch.zeros(B, D, dtype=torch.bool)
    hit[2] = True
    _only(I.ratios(got, want, A, I.c_rows(D)), hit, "l2_normalize")


def test_one_lost_pair_is_caught():
    B, F, D = 4, 39, 16
    e, g = one_signed((B, F, D), 1), one_signed((B, F * (F - 1) // 2), 2)
    want, A = I.pair_grad64(e, g)
    i, j = I.pairs(F)
    p = int(((i == 7) & (j == F - 1)).nonzero())
    g2 = g.clone()
    g2[1, p] = 0
    got, _ = I.pair_grad64(e, g2)
    hit = torch.zeros(B, F, D, dtype=torch.bool)
    hit[1, 7] = hit[1, F - 1] = True
    _only(I.ratios(got.float(), want, A, I.c_pair_bwd(F)), hit, "inner_product gradient")
    want, A = I.inner_product64(e)
    lost = _orc_modes(e, 2)
    lost[1, p] = 0
    hit = torch.zeros(want.shape, dtype=torch.bool)
    hit[1, p] = True
    _only(I.ratios(lost, want, A, I.c_inner(D)), hit, "inner_product")


def test_one_lost_history_step_is_caught():
    B, L, D = 4, 300, 16
    e = one_signed((B, L, D), 3)
    mask = torch.ones(B, L)
    lost = e.clone()
    lost[2, L - 1] = 0
    for denom in (0, 1, 2, 3):
        want, A = I.pool64(e, mask, True, denom, 1e-12)
        den = 1.0 if denom == 0 else float(L)
        got = (lost.cumsum(1)[:, -1] / den)                           # float32, in sequence
        hit = torch.zeros(B, D, dtype=torch.bool)
        hit[2] = True
        _only(I.ratios(got, want, A, I.c_pool(L)), hit, "pool denom %d" % denom)


def test_one_lost_element_of_pair_dot_is_caught():
    from oracle import c_oracle as C
    B, N, D = 3, 5, 1024
    u, v = one_signed((B, D), 1), one_signed((B, N, D), 2)
    want, A = I.pair_dot64(u, v, 0.5)
    lost = v.clone()
    lost[1, 3, D - 1] = 0
    out = np.zeros((B, N), dtype=np.float32)
    C.load().orc_pairdot_fwd(C.ptr(np.ascontiguousarray(u.numpy())), C.ptr(np.ascontiguousarray(lost.numpy())), B, N, D, 0.5,
                             C.ptr(out))
    hit = torch.zeros(B, N, dtype=torch.bool)
    hit[1, 3] = True
    _only(I.ratios(torch.from_numpy(out), want, A, I.c_rows(D)), hit, "pair_dot")
    g = one_signed((B, N), 4)
    (du, a_du), _ = I.pair_dot_grad64(u, v, g, 0.5)
    got = 0.5 * (g[:, :, None] * lost).sum(1)
    hit = torch.zeros(B, D, dtype=torch.bool)
    hit[1, D - 1] = True
    _only(I.ratios(got, du, a_du, I.c_rows(D)), hit, "pair_dot du")
