"""oracle/optim64.py against torch.optim in float64 (SGD, Adagrad, SparseAdam on sparse gradients; the dense rules where
torch refuses sparse gradients with weight decay), the step-size function against ``math`` in double, the float32
formulas of the kernel evaluated on the CPU against the bound, and the measurement T_POW was set from.  No GPU.

``table_and_state`` below is the builder tests/test_gpu_optim_forms.py starts every table from."""
import math

import pytest
import torch

from oracle import optim64 as O

EPS32 = O.EPS32
RULES = [O.SGD, O.ADAGRAD, O.ADAM]
HP = {O.SGD: dict(lr=0.05), O.ADAGRAD: dict(lr=0.05, eps=1e-10), O.ADAM: dict(lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8)}
POW_BASES = [0.5, 0.9, 0.999, 0.9999]
POW_T = list(range(1, 41)) + list(range(4990, 5011))


def gen(seed):
    return torch.Generator().manual_seed(seed)


def table_and_state(shape, g):
    """(w, s1, s2): state away from zero, so that a row that was read or written by mistake shows; second moments >= 0.5,
    so that A stays meaningful (1 / sqrt(v) of a v near zero magnifies one ulp of v)."""
    w = torch.randn(shape, generator=g).mul_(0.1)
    s1 = torch.rand(shape, generator=g).mul_(0.5).add_(0.25)
    s2 = torch.rand(shape, generator=g).add_(0.5)
    return w, s1, s2


def f32(v):
    return float(torch.tensor(float(v), dtype=torch.float32))


def _case(V=23, D=5, seed=0, n=9):
    g = gen(seed)
    w, s1, s2 = table_and_state((V, D), g)
    rows = torch.randperm(V, generator=g)[:n]
    grad = torch.zeros(V, D)
    grad[rows] = torch.randn(n, D, generator=g).div_(64)
    return w, s1, s2, grad, rows


def _torch_opt(kind, p, hp, wd=0.0):
    if kind == O.SGD:
        return torch.optim.SGD([p], lr=f32(hp["lr"]), weight_decay=wd)
    if kind == O.ADAGRAD:
        return torch.optim.Adagrad([p], lr=f32(hp["lr"]), eps=f32(hp["eps"]), weight_decay=wd)
    return torch.optim.SparseAdam([p], lr=f32(hp["lr"]), betas=(f32(hp["beta1"]), f32(hp["beta2"])), eps=f32(hp["eps"]))


@pytest.mark.parametrize("kind", RULES)
def test_sparse_rules_of_torch_optim_in_float64(kind):
    """Step t = 1, 2, 7 on a sparse float64 gradient, from a table and a state away from zero (torch's state is set to the
    oracle's inputs and its step counter to t - 1): table and state agree on every row, stepped or not."""
    hp = HP[kind]
    dec = 0.1 if kind == O.ADAGRAD else 0.0
    for t in (1, 2, 7):
        w, s1, s2, grad, rows = _case(seed=10 + t)
        rows = torch.sort(rows).values
        p = torch.nn.Parameter(w.double().clone())
        opt = _torch_opt(kind, p, hp)
        if kind == O.ADAGRAD:
            opt.param_groups[0]["lr_decay"] = f32(dec)
            opt.state[p]["sum"] = s1.double().clone()
            opt.state[p]["step"] = torch.tensor(float(t - 1))
        if kind == O.ADAM:
            opt.state[p].update(step=t - 1, exp_avg=s1.double().clone(), exp_avg_sq=s2.double().clone())
        p.grad = torch.sparse_coo_tensor(rows[None], grad[rows].double(), w.shape).coalesce()
        opt.step()
        lr_t, _ = O.step_size(kind, hp["lr"], hp.get("beta1", 0), hp.get("beta2", 0), dec, t)
        kw = dict((k, v) for k, v in hp.items() if k != "lr")
        # (lr_t is a double: the rule is linear in lr, so it is folded in exactly -- the comparison is at 1e-12)
        (got, _), (n1, _), (n2, _) = _step_exact(kind, w, grad, rows, s1, s2, lr_t, kw)
        err = float((p.detach() - got).abs().max())
        assert err <= 1e-12, (kind, t, err)
        if kind == O.ADAGRAD:
            assert float((opt.state[p]["sum"] - n1).abs().max()) <= 1e-12
        if kind == O.ADAM:
            assert float((opt.state[p]["exp_avg"] - n1).abs().max()) <= 1e-12
            assert float((opt.state[p]["exp_avg_sq"] - n2).abs().max()) <= 1e-12


def _step_exact(kind, w, g, rows, s1, s2, lr, kw, wd=0.0):
    """step_rows with a step size that is NOT rounded to float32: the rule is linear in lr, so step with lr = 1 scaled."""
    (w1, a), st1, st2 = O.step_rows(kind, w, g, rows, s1, s2, lr=1.0, weight_decay=wd, **kw)
    w64 = w.double()
    return (w64 + lr * (w1 - w64), a), st1, st2


@pytest.mark.parametrize("kind", RULES)
def test_weight_decay_against_the_dense_rules_on_a_batch_that_touches_every_row(kind):
    """torch refuses sparse gradients with weight_decay: the dense SGD / Adagrad (and, for Adam, the plain formulas of
    torch.optim.Adam with the bias correction folded into the step size) on a gradient that names every row."""
    V, D, wd = 11, 4, f32(0.03)
    g = gen(5)
    w = torch.randn(V, D, generator=g, dtype=torch.float64).float().double()
    grad = torch.randn(V, D, generator=g)
    hp = HP[kind]
    rows = torch.arange(V)
    p = torch.nn.Parameter(w.clone())
    if kind != O.ADAM:
        opt = _torch_opt(kind, p, hp, wd=wd)
    else:
        hp = dict(hp, eps=0.0)           # torch's dense Adam places eps differently: compared at eps = 0
        opt = torch.optim.Adam([p], lr=f32(hp["lr"]), betas=(f32(hp["beta1"]), f32(hp["beta2"])), eps=0.0, weight_decay=wd)
    p.grad = grad.double()
    opt.step()
    want = p.detach()
    lr_t, _ = O.step_size(kind, hp["lr"], hp.get("beta1", 0), hp.get("beta2", 0), 0.0, 1)
    kw = dict((k, v) for k, v in hp.items() if k != "lr")
    z = torch.zeros(V, D)
    (got, _), _, _ = _step_exact(kind, w, grad, rows, z, z, lr_t, kw, wd=wd)
    err = float((got - want).abs().max())
    assert err <= 1e-12, (kind, err)
    # and weight decay did something
    (plain, _), _, _ = _step_exact(kind, w, grad.float(), rows, z, z, lr_t, kw, wd=0.0)
    assert float((plain - got).abs().max()) > 1e-6


@pytest.mark.parametrize("kind", RULES)
def test_untouched_rows_duplicates_and_zero_gradient_rows(kind):
    w, s1, s2, grad, rows = _case(seed=3)
    hp = HP[kind]
    zero_row = int(rows[0])
    grad[zero_row] = 0.0                                   # looked up, summed gradient exactly zero
    once = O.step_rows(kind, w, grad, rows, s1, s2, **hp)
    twice = O.step_rows(kind, w, grad, torch.cat([rows, rows, rows[:3]]), s1, s2, **hp)
    for (a, aa), (b, ab) in zip(once, twice):
        assert (a is None and b is None) or (torch.equal(a, b) and torch.equal(aa, ab)), "a row named twice was stepped twice"
    mask = torch.zeros(w.shape[0], dtype=torch.bool)
    mask[rows] = True
    (w1, a_w), (n1, a1), (n2, a2) = once
    assert torch.equal(w1[~mask], w.double()[~mask]) and float(a_w[~mask].abs().max()) == 0.0
    assert bool((w1[mask] != w.double()[mask]).any())
    if kind == O.SGD:
        assert n1 is None and n2 is None
        assert torch.equal(w1[zero_row], w.double()[zero_row])          # SGD without weight decay: a zero step
    if kind == O.ADAGRAD:
        assert n2 is None and torch.equal(n1[~mask], s1.double()[~mask])
        assert torch.equal(n1[zero_row], s1.double()[zero_row]) and torch.equal(w1[zero_row], w.double()[zero_row])
    if kind == O.ADAM:
        assert torch.equal(n1[~mask], s1.double()[~mask]) and torch.equal(n2[~mask], s2.double()[~mask])
        # the zero-gradient row IS stepped: moments decay, w moves by the decayed first moment
        b1, b2, lr, eps = f32(0.9), f32(0.999), f32(hp["lr"]), f32(hp["eps"])
        m, v = s1.double()[zero_row], s2.double()[zero_row]
        assert torch.allclose(n1[zero_row], b1 * m, rtol=1e-14, atol=0) and torch.allclose(n2[zero_row], b2 * v, rtol=1e-14, atol=0)
        want = w.double()[zero_row] - lr * (b1 * m) / ((b2 * v).sqrt() + eps)
        assert torch.allclose(w1[zero_row], want, rtol=1e-14, atol=0)
        assert bool((w1[zero_row] != w.double()[zero_row]).all())


@pytest.mark.parametrize("kind", RULES)
def test_step_size_against_math_in_double(kind):
    lr, b1, b2, dec = f32(0.01), f32(0.9), f32(0.999), f32(0.1)
    for t in POW_T:
        got, K = O.step_size(kind, 0.01, 0.9, 0.999, 0.1, t)
        want = {O.SGD: lr, O.ADAGRAD: lr / (1 + (t - 1) * dec),
                O.ADAM: lr * math.sqrt(1 - math.pow(b2, t)) / (1 - math.pow(b1, t))}[kind]
        assert abs(got - want) <= 1e-15 * want, (kind, t)
        assert K >= 0.0
    got, K = O.step_size(O.ADAM, 0.01, 0.0, 0.999, 0.0, 7)          # b1 = 0: no bias correction of m, K stays finite
    assert abs(got - lr * math.sqrt(1 - b2 ** 7)) <= 1e-15 * got and math.isfinite(K)


def test_float32_pow_and_the_allowance():
    """T_POW: float32 pow on the CPU against float64 pow of the same float32 arguments, in ulps of the result."""
    worst = 0.0
    for b in POW_BASES:
        base = torch.tensor([b], dtype=torch.float32)
        for t in POW_T:
            got = float(torch.pow(base, torch.tensor([float(t)], dtype=torch.float32)))
            want = math.pow(float(base), t)
            ulp = float(torch.nextafter(torch.tensor(got), torch.tensor(2.0)) - torch.tensor(got))
            worst = max(worst, abs(got - want) / ulp)
    print("float32 pow: worst %.3f ulp; T_POW = %d" % (worst, O.T_POW))
    assert 4 * worst <= O.T_POW, "the 4x margin of T_POW is lost: measured %.3f ulp" % worst


def test_by_value_step_size_from_double_betas_is_outside_the_bound():
    """Verdict (a), second half: lr sqrt(1 - b2^t) / (1 - b1^t) from the DOUBLE 0.999 against the same from float32(0.999)
    differs by more than the bound the device's own arithmetic is held to -- which is why recbox_amd.optim rounds first."""
    worst, at = 0.0, None
    for t in list(range(1, 41)) + [100, 1000]:
        want, K = O.step_size(O.ADAM, 0.01, 0.9, 0.999, 0.0, t)
        dbl = f32(0.01) * math.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)
        r = abs(dbl - want) / (K * EPS32 * want)
        if r > worst:
            worst, at = r, (t, abs(dbl - want) / (EPS32 * want), K)
    print("double betas vs float32 betas: worst diff / bound %.2f at t = %d (%.1f eps32, K = %.1f)" % ((worst,) + at))
    assert worst > 1.0


@pytest.mark.parametrize("wd", [0.0, 0.05])
@pytest.mark.parametrize("kind", RULES)
def test_float32_formulas_stay_inside_the_bound(kind, wd):
    """The kernel's formulas (opt_apply) in torch float32 on the CPU against the oracle, on tables built like the GPU
    test's and a gradient at batch-mean scale -- with weight decay, gradients that nearly cancel wd w among them: the
    derivation of A holds with C_BOUND and no allowance (sqrt and / are correctly rounded)."""
    V, D = 257, 16
    g = gen(7 + kind)
    w, s1, s2 = table_and_state((V, D), g)
    grad = torch.randn(V, D, generator=g).div_(64)
    if wd:
        grad[:32] = -f32(wd) * w[:32] * (1 + torch.randn(32, D, generator=g) * 1e-3)      # g + wd w cancels to 1e-3
    grad[40:44] = 0.0
    hp = HP[kind]
    rows = torch.arange(0, V, 2)
    lr, b1, b2 = [torch.tensor(hp.get(k, 0.0), dtype=torch.float32) for k in ("lr", "beta1", "beta2")]
    eps, wdt = torch.tensor(hp.get("eps", 0.0), dtype=torch.float32), torch.tensor(wd, dtype=torch.float32)
    wr, gr, ar, br = w[rows], grad[rows], s1[rows].clone(), s2[rows].clone()
    gp = gr + wdt * wr
    if kind == O.SGD:
        wn = wr - lr * gp
    elif kind == O.ADAGRAD:
        ar = ar + gp * gp
        wn = wr - lr * gp / (ar.sqrt() + eps)
    else:
        ar = b1 * ar + (1 - b1) * gp
        br = b2 * br + (1 - b2) * gp * gp
        wn = wr - lr * ar / (br.sqrt() + eps)
    (w64, a_w), (n1, a1), (n2, a2) = O.step_rows(kind, w, grad, rows, s1, s2, weight_decay=wd, **hp)
    worst = float(((wn.double() - w64[rows]).abs() / (EPS32 * a_w[rows] + O.TINY)).max())
    if n1 is not None:
        worst = max(worst, float(((ar.double() - n1[rows]).abs() / (EPS32 * a1[rows] + O.TINY)).max()))
    if n2 is not None:
        worst = max(worst, float(((br.double() - n2[rows]).abs() / (EPS32 * a2[rows] + O.TINY)).max()))
    print("rule %d wd %g: float32 formulas worst %.2f x eps32 A (C = %d)" % (kind, wd, worst, O.C_BOUND))
    assert 4 * worst <= O.C_BOUND
