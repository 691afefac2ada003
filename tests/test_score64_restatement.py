"""oracle/score64.py against torch float64 autograd (1e-12 relative), its edge cases (padding row, out-of-range id, zero
row, -inf / -1e9 candidates, saturated logits), sigmoid_bce against torch's float32 BCE where clamp and saturation must
coincide exactly, and the float32-on-the-CPU measurement the transcendental allowance T_ALLOW was set from.  No GPU.

The input builders below are the ones tests/test_gpu_score_forms.py runs the kernels on."""
import pytest
import torch
import torch.nn.functional as F

from oracle import score64 as S
from test_interact64_restatement import one_signed, randn

EPS32 = S.EPS32
LADDER = [-110.0, -88.0, -20.0, -17.0, 0.0, 16.0, 17.0, 20.0, 88.0, 110.0]
SATURATED = [17.0, 20.0, 88.0, 110.0]          # 1 / (1 + expf(-x)) == 1.0f
BCE_POINTS = [0.0, 1.0, 1e-30, 1.0 - 2.0 ** -24]
BCE_Y = [0.0, 1.0, 0.3]


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- input builders (shared with the GPU file) ------------------------------------------------------------------------
def dot_case(D, widths=(1, 2), V=50, R=257, seed=0, kind="randn", shared=False):
    """x [R, D], two tables [V, D], id sets of the given widths: sets 0 and 2.. share table 0, set 1 has its own (or shares
    table 0 as well); set 0 is int32, the others int64."""
    make = {"randn": randn, "one_signed": one_signed}[kind]
    x = make((R, D), seed * 7 + D)
    tabs = [make((V, D), seed * 7 + D + 1 + i) * 0.5 for i in range(2)]
    g = gen(seed * 7 + D + 5)
    sets, tables = [], []
    for i, w in enumerate(widths):
        ids = torch.randint(0, V, (R,) if w == 1 and i == 0 else (R, w), generator=g)
        sets.append(ids.int() if i == 0 else ids)
        tables.append(tabs[1] if (i == 1 and not shared) else tabs[0])
    gout = torch.randn(R, sum(widths), generator=g)
    return x, tables, sets, gout


def cos_case(D, N, B=37, seed=0, kind="randn"):
    """u [B, D] normalised, v [B, N, D] with one zero row (b = 1, n = 0) and one row of norm 1e-20 (b = 2, n = N - 1)."""
    make = {"randn": randn, "one_signed": one_signed}[kind]
    u = F.normalize(make((B, D), seed * 11 + D), dim=-1)
    v = make((B, N, D), seed * 11 + D + 1).clone()
    v[1, 0] = 0.0
    v[2, N - 1] = F.normalize(v[2, N - 1], dim=-1) * 1e-20
    g = torch.randn(B, N, generator=gen(seed * 11 + D + 2))
    return u, v, g


def sce_case(kind, rows, n, seed=0, target="random"):
    g = gen(seed * 13 + rows + n)
    t = {"none": None, "random": torch.randint(0, n, (rows,), generator=g),
         "last": torch.full((rows,), n - 1, dtype=torch.long)}[target]
    if kind == "randn4":
        x = torch.randn(rows, n, generator=g) * 4
    elif kind == "uniform100":
        x = torch.rand(rows, n, generator=g) * 200 - 100
    elif kind == "constant":
        x = (torch.randn(rows, 1, generator=g) * 4).expand(rows, n).clone()
    else:                                           # "masked": -1e9 and -inf away from the target
        x = torch.randn(rows, n, generator=g) * 4
        sel = torch.rand(rows, n, generator=g)
        tt = torch.zeros(rows, dtype=torch.long) if t is None else t
        away = torch.ones(rows, n, dtype=torch.bool).scatter_(1, tt[:, None], False)
        x[away & (sel < 0.3)] = -1e9
        x[away & (sel >= 0.3) & (sel < 0.5)] = float("-inf")
    return x, t


def pair_case(kind, n, seed=0, weight="none"):
    g = gen(seed * 17 + n)
    if kind == "randn6":
        pos, neg = torch.randn(n, generator=g) * 6, torch.randn(n, generator=g) * 6
    else:
        pos, neg = torch.rand(n, generator=g) * 200 - 100, torch.rand(n, generator=g) * 200 - 100
    if weight == "none":
        w = None
    elif weight == "mask":                          # 0 / 1 over the count
        m = (torch.rand(n, generator=g) < 0.7).float()
        w = m / max(float(m.sum()), 1.0)
    else:
        w = torch.rand(n, generator=g) * 2 + 0.01
    return pos, neg, w


def bce_case(n, seed=0):
    """p inside [1e-6, 1 - 1e-6]; the first 12 elements (as n allows) are BCE_POINTS x BCE_Y."""
    g = gen(seed * 19 + n)
    p = (torch.rand(n, generator=g).double() * (1 - 2e-6) + 1e-6).float().clamp(1e-6, 1 - 1e-6)
    y = (torch.rand(n, generator=g) < 0.3).float()
    y[torch.rand(n, generator=g) < 0.1] = 0.3
    pts = [(pp, yy) for pp in BCE_POINTS for yy in BCE_Y][:n]
    for i, (pp, yy) in enumerate(pts):
        p[i], y[i] = pp, yy
    return p, y


def sigmoid_case(n, seed=0):
    """logits randn * 3 with the ladder (each rung twice: y = 0 and y = 1) at the front, as n allows."""
    g = gen(seed * 23 + n)
    x = torch.randn(n, generator=g) * 3
    y = (torch.rand(n, generator=g) < 0.3).float()
    y[torch.rand(n, generator=g) < 0.1] = 0.3
    pts = [(xx, yy) for yy in (0.0, 1.0) for xx in LADDER][:n]
    for i, (xx, yy) in enumerate(pts):
        x[i], y[i] = xx, yy
    return x, y


def rel(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return float(((a - b).abs() / b.abs().clamp_min(1e-300)).max()) if a.numel() else 0.0


def close12(a, b, what, A=None):
    """1e-12 relative: to the value, or, where the terms cancel (a gradient that subtracts), to their absolute sum A."""
    a, b = a.double(), b.double().reshape(a.shape)
    err = (a - b).abs()
    assert bool((err <= 1e-12 * (b.abs() if A is None else A) + 1e-300).all()), "%s: %.3g relative" % (what, rel(a, b))


# ---- against float64 autograd -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 16, 65])
def test_gather_dot_against_autograd_with_padding_row(D):
    x, tables, sets, gout = dot_case(D, widths=(1, 2, 2), R=64)
    pad = 3
    xd = x.double().requires_grad_(True)
    uniq = [tables[0].double().requires_grad_(True), tables[1].double().requires_grad_(True)]
    td = [uniq[1] if t is tables[1] else uniq[0] for t in tables]
    cols = [(xd[:, None, :] * F.embedding(i.long().reshape(64, -1), w, padding_idx=pad)).sum(-1) * 0.25 for w, i in zip(td, sets)]
    ref = torch.cat(cols, 1)
    (ref * gout.double()).sum().backward()
    out, A = S.gather_dot(x, tables, sets, 0.25, pad)
    (dx, a_dx), grads = S.gather_dot_grad(x, tables, sets, gout, 0.25, pad)
    close12(out, ref.detach(), "out")
    close12(dx, xd.grad, "dx", a_dx)
    for (dw, a), w in zip(grads, uniq):
        close12(dw, w.grad, "dW", a)
        assert int(dw[pad].count_nonzero()) == 0 and int(a[pad].count_nonzero()) == 0
    assert bool((A >= out.abs() * (1 - 1e-12)).all()) and bool((a_dx >= dx.abs() * (1 - 1e-12)).all())
    assert any(bool((i.long() == pad).any()) for i in sets)
    hit = (sets[0].long() == pad)
    assert bool((out[hit, 0] != 0).all())           # the padding row is scored as the row it is


def test_gather_dot_out_of_range_id_scores_zero_and_has_no_gradient():
    x, tables, sets, gout = dot_case(8, widths=(1, 2), R=32)
    good = S.gather_dot_grad(x, tables, [sets[0], sets[1]], gout)
    bad1 = sets[1].clone()
    bad1[5, 0], bad1[6, 1] = 50, -1
    out, A = S.gather_dot(x, tables, [sets[0], bad1])
    assert float(out[5, 1]) == 0 and float(out[6, 2]) == 0 and float(A[5, 1]) == 0 and float(A[6, 2]) == 0
    g2 = gout.clone()
    g2[5, 1], g2[6, 2] = 0.0, 0.0                    # the same gradients as in-range ids whose upstream gradient is zero
    (dx, _), grads = S.gather_dot_grad(x, tables, [sets[0], bad1], gout)
    (dx2, _), grads2 = S.gather_dot_grad(x, tables, [sets[0], sets[1]], g2)
    assert torch.equal(dx, dx2) and all(torch.equal(a[0], b[0]) for a, b in zip(grads, grads2))
    assert not torch.equal(dx, good[0][0])


@pytest.mark.parametrize("kind", ["randn", "one_signed"])
@pytest.mark.parametrize("D,N", [(4, 1), (12, 5), (1000, 5)])
def test_cos_dot_against_autograd(D, N, kind):
    u, v, g = cos_case(D, N, B=9, kind=kind)
    ud, vd = u.double().requires_grad_(True), v.double().requires_grad_(True)
    eps = float(torch.tensor(1e-12, dtype=torch.float32))
    ref = 20.0 * (ud[:, None, :] * F.normalize(vd, p=2, dim=-1, eps=eps)).sum(-1)
    (ref * g.double()).sum().backward()
    out, A = S.cos_dot(u, v, 1e-12, 20.0)
    (du, a_du), (dv, a_dv) = S.cos_dot_grad(u, v, g, 1e-12, 20.0)
    close12(out, ref.detach(), "out")
    close12(du, ud.grad, "du", a_du)
    close12(dv, vd.grad, "dv", a_dv)
    assert float(out[1, 0]) == 0 and float(A[1, 0]) == 0                    # the zero row
    assert bool((a_dv >= dv.abs() * (1 - 1e-9)).all()) and bool((a_du >= du.abs() * (1 - 1e-9)).all())
    want = 20.0 * float(g[1, 0]) * u[1].double() / eps                        # ... whose dv is autograd's g u / eps
    close12(dv[1, 0], want, "dv of the zero row")
    zu = u.clone()
    zu[3] = 0.0                                                                # a zero user row: 0 and a zero gradient
    o2, A2 = S.cos_dot(zu, v, 1e-12, 20.0)
    (_, _), (dv2, a2) = S.cos_dot_grad(zu, v, g, 1e-12, 20.0)
    assert int(o2[3].count_nonzero()) == 0 and int(A2[3].count_nonzero()) == 0
    assert int(dv2[3].count_nonzero()) == 0 and int(a2[3].count_nonzero()) == 0


@pytest.mark.parametrize("target", ["none", "random", "last"])
@pytest.mark.parametrize("kind", ["randn4", "uniform100", "constant", "masked"])
@pytest.mark.parametrize("n", [1, 2, 5, 101])
def test_softmax_ce_against_autograd(n, kind, target):
    x, t = sce_case(kind, 33, n, target=target)
    xd = x.double().requires_grad_(True)
    tt = torch.zeros(33, dtype=torch.long) if t is None else t
    ref = F.cross_entropy(xd, tt)
    ref.backward()
    (loss, A), (lse, a_lse) = S.softmax_ce(x, t)
    dx, a_dx = S.softmax_ce_grad(x, t, 1.0)
    close12(loss, ref.detach(), "loss")
    close12(lse, torch.logsumexp(x.double(), 1), "lse")
    close12(dx, xd.grad, "dlogits", a_dx)
    assert bool(torch.isfinite(A)) and bool(torch.isfinite(a_dx).all()) and bool(torch.isfinite(a_lse).all())
    gone = torch.isinf(x)
    assert int(dx[gone].count_nonzero()) == 0 and int(a_dx[gone].count_nonzero()) == 0
    if kind == "masked" and n > 1:
        assert bool(gone.any()) and bool((x == -1e9).any())
        keep = x.clone()
        keep[gone] = -1e30                          # -inf adds exactly 0: the loss of the rows without those entries
        assert float(S.softmax_ce(keep, t)[0][0]) == float(loss)
    if n == 1:
        assert float(loss) == 0 and int(dx.count_nonzero()) == 0


@pytest.mark.parametrize("weight", ["none", "mask", "positive"])
@pytest.mark.parametrize("kind", ["randn6", "uniform100"])
def test_pair_logsigmoid_against_autograd_and_masked_positions(kind, weight):
    pos, neg, w = pair_case(kind, 1025, weight=weight)
    pd, nd = pos.double().requires_grad_(True), neg.double().requires_grad_(True)
    wd = torch.ones(1025, dtype=torch.float64) if w is None else w.double()
    ref = 0.5 * (-wd * (F.logsigmoid(pd) + F.logsigmoid(-nd))).sum()
    (ref * 3.0).backward()
    (loss, A), _ = S.pair_logsigmoid(pos, neg, w, 0.5)
    (dp, a_dp), (dn, a_dn) = S.pair_logsigmoid_grad(pos, neg, w, 0.5, 3.0)
    close12(loss, ref.detach(), "loss")
    assert bool(((dp - pd.grad).abs() <= 1e-12 * a_dp + 1e-300).all())
    assert bool(((dn - nd.grad).abs() <= 1e-12 * a_dn + 1e-300).all())
    if weight == "mask":
        dead = w == 0
        assert bool(dead.any())
        p2, n2 = pos.clone(), neg.clone()
        idx = dead.nonzero().reshape(-1)
        p2[idx[0::3]], n2[idx[1::3]], p2[idx[2::3]] = float("inf"), float("-inf"), float("nan")
        n2[idx[0::3]] = float("nan")
        (loss2, A2), _ = S.pair_logsigmoid(p2, n2, w, 0.5)
        (dp2, a2), (dn2, b2) = S.pair_logsigmoid_grad(p2, n2, w, 0.5, 3.0)
        assert float(loss2) == float(loss) and float(A2) == float(A)
        assert torch.equal(dp2, dp) and torch.equal(dn2, dn)
        assert int(dp2[dead].count_nonzero()) == 0 and int(dn2[dead].count_nonzero()) == 0
        assert int(a2[dead].count_nonzero()) == 0 and int(b2[dead].count_nonzero()) == 0


def test_bce_against_autograd_clamp_and_guard():
    p, y = bce_case(1025)
    pd = p.double().requires_grad_(True)
    ref = F.binary_cross_entropy(pd, y.double())
    ref.backward()
    (loss, A), (term, a) = S.bce(p, y)
    dp, a_dp = S.bce_grad(p, y, 1.0)
    close12(loss, ref.detach(), "loss")
    # torch's float64 guard is the double 1e-12; the kernels' is the float32 one: the two differ in the 9th digit
    inside = ((1 - p.double()) * p.double()) > 2e-12
    close12(dp[inside], pd.grad[inside], "dp")
    assert bool(((dp[~inside] - pd.grad[~inside]).abs() <= 1e-7 * dp[~inside].abs()).all())
    pts = [(pp, yy) for pp in BCE_POINTS for yy in BCE_Y]
    for i, (pp, yy) in enumerate(pts):
        if pp == 0.0:
            assert float(term[i]) == 100.0 * float(y[i].double())
            assert float(dp[i]) == (0.0 - float(y[i].double())) / 1025 / S.F32_GUARD
        if pp == 1.0:
            assert float(term[i]) == 100.0 * (1.0 - float(y[i].double()))


def test_sigmoid_bce_against_float32_torch_clamp_and_saturation_coincide():
    x, y = sigmoid_case(1025)
    o = S.sigmoid_bce(x, y, 2.0)
    x32 = x.clone().requires_grad_(True)
    p32 = torch.sigmoid(x32)
    terms32 = F.binary_cross_entropy(p32, y, reduction="none")
    (2.0 * terms32.mean()).backward()
    p64, term, dx = o["prob"][0], o["terms"][0], o["dx"][0]
    same = p64 == p32.detach().double()
    # the two probabilities agree to two ulp everywhere, and bit for bit on every rung but the knife edge x = 17
    assert bool(((p64 - p32.detach().double()).abs() <= 2 * S._ulp32(p64)).all())
    for i, xx in enumerate(LADDER + LADDER):         # which rungs saturate: x >= 17 in float32, x >= 20 after the rounding
        assert (float(p32[i].detach()) == 1.0) == (xx in SATURATED) and (float(p64[i]) == 1.0) == (xx in SATURATED[1:]), xx
        assert (float(p32[i].detach()) == 0.0) == (xx == -110.0) and (float(p64[i]) == 0.0) == (xx == -110.0), xx
    assert not bool(same[LADDER.index(17.0)])
    assert float(p64[LADDER.index(17.0)]) == 1.0 - 2.0 ** -24 and float(p32.detach()[LADDER.index(17.0)]) == 1.0
    # ... and on torch's float32 probabilities the restatement coincides exactly in clamp and saturation
    q = S.sigmoid_bce(x, y, 2.0, p32=p32.detach())
    sat = p32.detach() == 1.0
    assert int(sat.sum()) >= 2 * len(SATURATED)
    assert torch.equal(q["terms"][0][sat], 100.0 * (1.0 - y.double()[sat]))
    assert torch.equal(terms32.detach().double()[sat], 100.0 * (1.0 - y.double()[sat]))
    assert int(q["dx"][0][sat].count_nonzero()) == 0 and int(x32.grad[sat].count_nonzero()) == 0
    zero = p32.detach() == 0.0
    assert bool(zero.any())
    assert torch.equal(q["terms"][0][zero], 100.0 * y.double()[zero])
    assert torch.equal(terms32.detach().double()[zero], 100.0 * y.double()[zero])
    assert int(q["dx"][0][zero].count_nonzero()) == 0 and int(x32.grad[zero].count_nonzero()) == 0
    r = (q["terms"][0] - terms32.detach().double()).abs() / (8 * EPS32 * q["terms"][1] + 1e-30)
    assert float(r.max()) <= 1.0
    r = (q["dx"][0] - x32.grad.double()).abs() / (8 * EPS32 * q["dx"][1] + 1e-30)
    assert float(r.max()) <= 1.0
    # where the two probabilities are ONE ulp apart the default evaluation differs by at most ``cond``, the knife edge included
    one = (p64 - p32.detach().double()).abs() <= S._ulp32(p64)
    assert bool(one[LADDER.index(17.0)]) and int(one.sum()) > 900
    assert bool(((term - q["terms"][0]).abs()[one] <= o["terms"][2][one] * (1 + 1e-6) + 1e-300).all())
    assert bool(((dx - q["dx"][0]).abs()[one] <= o["dx"][2][one] * (1 + 1e-6) + 1e-300).all())
    edge = LADDER.index(17.0)                        # y = 0 there: 16.6 against the clamp's 100
    assert abs(float(term[edge]) - 24 * 0.6931471805599453) < 1e-9 and float(q["terms"][0][edge]) == 100.0
    # away from saturation cond is the first-order ulp / p, ulp / (1 - p)
    mid = (p64 > 0.01) & (p64 < 0.99)
    lin = S._ulp32(p64) * (y.double().abs() / p64 + (1 - y.double()).abs() / (1 - p64))
    assert bool(((o["terms"][2][mid] - lin[mid]).abs() <= 1e-4 * lin[mid]).all())


# ---- the float32 formulas on the CPU: what T_ALLOW was set from -------------------------------------------------------
def f32_softmax(x, t):
    x = x.float()
    m = x.max(1, keepdim=True).values
    s = torch.exp(x - m).double().sum(1, keepdim=True).float()     # (the sum itself belongs to the structural part)
    lse = (m + torch.log(s)).squeeze(1)
    p = torch.exp(x - lse[:, None])
    hot = torch.zeros_like(p).scatter_(1, t[:, None], 1.0)
    return lse, (p - hot) / x.shape[0]


def f32_logsig(v):
    return torch.clamp_max(v, 0.0) - torch.log1p(torch.exp(-v.abs()))


def f32_sigmoid_bce(x, y, gs):
    x, y = x.float(), y.float()
    p = 1.0 / (1.0 + torch.exp(-x))
    lp, lq = torch.log(p).clamp_min(-100.0), torch.log1p(-p).clamp_min(-100.0)
    q = (1.0 - p) * p
    dx = torch.tensor(gs / x.numel(), dtype=torch.float32) * (p - y) / q.clamp_min(1e-12) * q
    return p, -(y * lp + (1.0 - y) * lq), dx


def measure():
    """{label: worst err / (eps32 A)} of the float32 formulas, element by element, on the GPU file's inputs."""
    worst = {}

    def note(label, got, want, A):
        live = A > 0
        r = ((got.double() - want).abs()[live] / (EPS32 * A[live] + 1e-30)).max() if bool(live.any()) else 0.0
        worst[label] = max(worst.get(label, 0.0), float(r))

    for kind in ("randn4", "uniform100", "constant", "masked"):
        for n in (2, 5, 101):
            x, t = sce_case(kind, 257, n)
            lse, dx = f32_softmax(x, t)
            (_, _), (w_lse, a_lse) = S.softmax_ce(x, t)
            w_dx, a_dx = S.softmax_ce_grad(x, t, 1.0)
            note("softmax lse", lse, w_lse, a_lse)
            note("softmax dx", dx, w_dx, a_dx)
    for kind in ("randn6", "uniform100"):
        pos, neg, w = pair_case(kind, 1025, weight="positive")
        term = -w * (f32_logsig(pos) + f32_logsig(-neg))
        _, (w_term, a_term) = S.pair_logsigmoid(pos, neg, w, 1.0)
        note("pair term", term, w_term, a_term)
        sp, sn = 1.0 / (1.0 + torch.exp(-pos)), 1.0 / (1.0 + torch.exp(-neg))
        (dp, a_dp), (dn, a_dn) = S.pair_logsigmoid_grad(pos, neg, w, 1.0, 1.0)
        note("pair gradients", -w * (1.0 - sp), dp, a_dp)
        note("pair gradients", w * sn, dn, a_dn)
    p, y = bce_case(1025)
    term = -(y * torch.log(p).clamp_min(-100.0) + (1.0 - y) * torch.log1p(-p).clamp_min(-100.0))
    _, (w_term, a_term) = S.bce(p, y)
    note("bce term", term, w_term, a_term)
    x, y = sigmoid_case(1025)
    p, term, dx = f32_sigmoid_bce(x, y, 2.0)
    o = S.sigmoid_bce(x, y, 2.0)
    away = o["prob"][0] > 1e-37                      # (float32 subnormals: an absolute, not a relative, matter)
    note("sigmoid prob", p[away], o["prob"][0][away], o["prob"][1][away])
    q = S.sigmoid_bce(x, y, 2.0, p32=p)               # on the SAME probabilities: the log terms and dx alone
    note("sigmoid_bce term", term, q["terms"][0], q["terms"][1])
    note("sigmoid_bce dx", dx, q["dx"][0], q["dx"][1])
    return worst


def test_float32_formulas_and_the_allowance():
    worst = measure()
    print(", ".join("%s %.2f" % kv for kv in sorted(worst.items())))
    assert 4.0 * max(worst.values()) <= S.T_ALLOW, worst
