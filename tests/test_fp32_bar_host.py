"""The bar of tests/fp32_bar.py has teeth, shown on the CPU: for the GRU, the additive attention pooling and the capsule
routing, restated with hand-written backward passes (the formulas in the headers of csrc/rbx_gru.hip, rbx_addattn.hip and
rbx_capsule.hip),

  * the float32 restatement passes the bar against float64 on every tensor, and the hand-written float64 backward agrees with
    autograd over tests/gru64.py / addattn64.py / capsule64.py to 1e-12 of the tensor's size (so a mutation below is the only
    thing wrong with a mutant);
  * every mutant -- one deliberately wrong term, computed in float64 -- FAILS the bar on at least one tensor and PASSES the
    old absolute 1e-4 on every tensor.  Both halves are asserted: the old rule hid exactly these errors.

The upstream gradients are ~ N(0, 1) * 3e-6 (GRU), * 1e-5 (capsule) and * 3e-5 / sqrt(B) (additive attention): every gradient is
then below 1e-4 in magnitude, which is where the GPU tests' per-element gradients of large batches sit (1 / sqrt(B L) upstream),
and an absolute 1e-4 cannot see any error in them at all, while the bar follows the tensor's size down.  The additive
attention case takes v = -2 |v| of addattn64.make_case: the logits are then around -4, sum_l exp(q) of the sample of length 1
is about 0.02, and a denominator of ``sum + 1e-6`` moves its alpha by a few 1e-5 -- under 1e-4, far over 2e-6.  With v as
drawn (sum about 1) that mutant moves alpha by 1e-6, inside the floor of the bar: at O(1) sums it is not distinguishable from
fp32 rounding, and the draw above is what makes it so.

Mutants kept: GRU db_hh_n without r, a frozen step that lets dh pick up d_out, dh0 without the z carry of step 0 (the last
one the backward walks); additive attention dq without - G, dv without the last sample, alpha over sum + 1e-6; capsule squash
derivative without its 1 / (1 + |s|^2)^2 term, dW without the last sample.  Dropped: the capsule softmax renormalised over
the kept positions -- it moves the OUTPUT by several 1e-2, so the old 1e-4 catches it as well and the second half does not
hold (no upstream scale reaches a forward result)."""
import pytest
import torch

import addattn64
import capsule64
import gru64
from fp32_bar import assert_bar, within_absolute, within_bar

GRU_NAMES = ("out", "h_n", "dx", "dW_ih", "dW_hh", "db_ih", "db_hh", "dh0")
CAP_NAMES = ("out", "dx", "dW")


# ---- GRU ------------------------------------------------------------------------------------------------------------------------
def gru_case(B=17, L=7, I=16, H=20, up=3e-6):
    g = torch.Generator().manual_seed(1234)
    bound = 1.0 / H ** 0.5
    uni = lambda *s: (torch.rand(*s, generator=g) * 2 - 1) * bound
    lengths = torch.randint(0, L + 1, (B,), generator=g)
    lengths[0], lengths[1], lengths[2] = 0, L, 1
    return {"x": torch.randn(B, L, I, generator=g), "w_ih": uni(3 * H, I), "w_hh": uni(3 * H, H), "b_ih": uni(3 * H),
            "b_hh": uni(3 * H), "h0": torch.randn(B, H, generator=g), "lengths": lengths,
            "d_out": torch.randn(B, L, H, generator=g) * up, "d_hn": torch.randn(B, H, generator=g) * up}


def gru_autograd(case, dtype):
    leaves = [case[n].to(dtype).requires_grad_(True) for n in ("x", "w_ih", "w_hh", "b_ih", "b_hh", "h0")]
    out, hn = gru64.gru_layer(leaves[0], leaves[1], leaves[2], leaves[3], leaves[4], leaves[5], case["lengths"])
    grads = torch.autograd.grad((out * case["d_out"].to(dtype)).sum() + (hn * case["d_hn"].to(dtype)).sum(), leaves)
    return dict(zip(GRU_NAMES, (out.detach(), hn.detach()) + tuple(grads)))


def gru_manual(case, dtype, bug=None):
    """Forward and the backward of rbx_gru.hip's header, step by step."""
    x, w_ih, w_hh, b_ih, b_hh, h0, d_out, d_hn = (case[n].to(dtype) for n in
                                                  ("x", "w_ih", "w_hh", "b_ih", "b_hh", "h0", "d_out", "d_hn"))
    lengths = case["lengths"]
    B, L, _ = x.shape
    H = w_hh.shape[1]
    gi = x @ w_ih.t() + b_ih
    h, saved, outs = h0, [], []
    for t in range(L):
        gh = h @ w_hh.t() + b_hh
        r = torch.sigmoid(gi[:, t, :H] + gh[:, :H])
        z = torch.sigmoid(gi[:, t, H:2 * H] + gh[:, H:2 * H])
        ghn = gh[:, 2 * H:]
        n = torch.tanh(gi[:, t, 2 * H:] + r * ghn)
        new = (1 - z) * n + z * h
        act = (lengths > t).unsqueeze(1)
        saved.append((r, z, n, ghn, h, act))
        h = torch.where(act, new, h)
        outs.append(torch.where(act, new, torch.zeros_like(new)))
    dh = d_hn.clone()
    dgi = torch.zeros(B, L, 3 * H, dtype=dtype)
    dgh = torch.zeros(B, L, 3 * H, dtype=dtype)
    dnp_all = torch.zeros(B, L, H, dtype=dtype)
    hp_all = torch.stack([s[4] for s in saved], dim=1)
    for t in reversed(range(L)):
        r, z, n, ghn, hp, act = saved[t]
        a = act.to(dtype)
        g = dh + d_out[:, t]
        dnp = g * (1 - z) * (1 - n * n) * a
        d_r = dnp * ghn * r * (1 - r)
        d_z = g * (hp - n) * z * (1 - z) * a
        dgi[:, t] = torch.cat([d_r, d_z, dnp], dim=1)
        dgh[:, t] = torch.cat([d_r, d_z, dnp * r], dim=1)
        dnp_all[:, t] = dnp
        frozen = dh + d_out[:, t] if bug == "frozen step takes d_out" else dh
        carry = torch.where(act, g * z, frozen)
        if bug == "dh0 without the z carry" and t == 0:
            carry = torch.where(act, torch.zeros_like(carry), frozen)
        dh = carry + dgh[:, t] @ w_hh
    db_hh = dgh.sum((0, 1))
    if bug == "db_hh_n without r":
        db_hh = torch.cat([db_hh[:2 * H], dnp_all.sum((0, 1))])
    res = (torch.stack(outs, dim=1), h, dgi @ w_ih, torch.einsum("blg,bli->gi", dgi, x),
           torch.einsum("blg,blh->gh", dgh, hp_all), dgi.sum((0, 1)), db_hh, dh)
    return dict(zip(GRU_NAMES, res))


GRU_BUGS = ("db_hh_n without r", "frozen step takes d_out", "dh0 without the z carry")


# ---- additive attention ---------------------------------------------------------------------------------------------------------
def addattn_case(B=17, L=17, D=20, H=12, up=3e-5):
    case = dict(addattn64.make_case(B, L, D, H, seed=11))
    case["v"] = -2.0 * case["v"].abs()
    case["g_out"] = case["g_out"] * up
    return case


def addattn_manual(case, dtype, bug=None):
    x, w, ctx, v, g_out = (case[n].to(dtype) for n in ("x", "w", "ctx", "v", "g_out"))
    keep = (case["mask"] != 0).to(dtype)
    s = torch.sigmoid(x @ w.t() + ctx.unsqueeze(1))                            # [B, L, H]
    e = torch.exp(s @ v) * keep
    total = e.sum(1, keepdim=True)
    alpha = e / (total + 1e-6 if bug == "alpha over sum + 1e-6" else total)
    out = (alpha.unsqueeze(-1) * x).sum(1)
    gl = torch.einsum("bd,bld->bl", g_out, x)
    G = (alpha * gl).sum(1, keepdim=True)
    dq = alpha * gl if bug == "dq without - G" else alpha * (gl - G)
    dpre = dq.unsqueeze(-1) * v * s * (1 - s)
    dvs = dq.unsqueeze(-1) * s
    dv = (dvs[:-1] if bug == "dv without the last sample" else dvs).sum((0, 1))
    res = (out, alpha, alpha.unsqueeze(-1) * g_out.unsqueeze(1) + dpre @ w, torch.einsum("blh,bld->hd", dpre, x),
           dpre.sum(1), dv)
    named = dict(zip(addattn64.NAMES, res))
    named["dpre"] = dpre                      # the transient of rbx_addattn_bwd (tests/test_gpu_addattn_forms.py compares it)
    return named


ADDATTN_BUGS = ("dq without - G", "dv without the last sample", "alpha over sum + 1e-6")


# ---- capsule routing, bilinear type 2 -------------------------------------------------------------------------------------------
def capsule_case(B=17, L=7, D=16, K=4, up=1e-5):
    g = torch.Generator().manual_seed(4321)
    lengths = torch.randint(0, L + 1, (B,), generator=g)
    lengths[0], lengths[1], lengths[B - 1] = 0, 1, L
    return {"x": torch.randn(B, L, D, generator=g), "w": torch.randn(1, L, K * D, D, generator=g) / D ** 0.5,
            "mask": (torch.arange(L).unsqueeze(0) < lengths.unsqueeze(1)).long(), "K": K,
            "r": torch.randn(B, K, D, generator=g) * up}


def capsule_autograd(case, dtype):
    x, w = (case[n].to(dtype).requires_grad_(True) for n in ("x", "w"))
    out = capsule64.capsule_forward(x, case["mask"], w, 2, case["K"])
    dx, dw = torch.autograd.grad((out * case["r"].to(dtype)).sum(), (x, w))
    return dict(zip(CAP_NAMES, (out.detach(), dx, dw)))


def capsule_manual(case, dtype, bug=None):
    """Two logit updates over hat as a constant, the output iteration, and the backward of rbx_capsule.hip's header."""
    x, w, dv = (case[n].to(dtype) for n in ("x", "w", "r"))
    K = case["K"]
    B, L, D = x.shape
    keep = (case["mask"] != 0).to(dtype).reshape(B, 1, L)
    wl = w.reshape(L, K * D, D)
    hat = torch.einsum("lnd,bld->bln", wl, x).reshape(B, L, K, D).transpose(1, 2)        # [B, K, L, D]
    z = torch.zeros(B, K, L, dtype=dtype)
    for it in range(3):
        c = torch.softmax(z, dim=-1) * keep
        s = torch.einsum("bkl,bkld->bkd", c, hat)
        n = (s * s).sum(-1, keepdim=True)
        rs = 1 / torch.sqrt(n + 1e-9)
        f = n / (1 + n) * rs
        v = f * s
        if it < 2:
            z = z + torch.einsum("bkld,bkd->bkl", hat, v)
    fp = -0.5 * n / (1 + n) * rs ** 3
    if bug != "squash derivative without 1 / (1 + n)^2":
        fp = fp + rs / (1 + n) ** 2
    ds = f * dv + 2 * fp * (s * dv).sum(-1, keepdim=True) * s
    dhat = (c.unsqueeze(-1) * ds.unsqueeze(2)).transpose(1, 2).reshape(B, L, K * D)      # [B, L, N]
    last = B - 1 if bug == "dW without the last sample" else B
    dw = torch.einsum("bln,bld->lnd", dhat[:last], x[:last]).reshape(w.shape)
    return dict(zip(CAP_NAMES, (v, torch.einsum("bln,lnd->bld", dhat, wl), dw)))


CAPSULE_BUGS = ("squash derivative without 1 / (1 + n)^2", "dW without the last sample")

FAMILIES = {"gru": (gru_case, gru_autograd, gru_manual, GRU_NAMES),
            "addattn": (addattn_case, lambda case, dtype: _addattn_autograd(case, dtype), addattn_manual, addattn64.NAMES),
            "capsule": (capsule_case, capsule_autograd, capsule_manual, CAP_NAMES)}


def _addattn_autograd(case, dtype):
    if dtype == torch.float64:
        return addattn64.reference(case)
    return addattn64.run(addattn64.forward, case)


_CACHE = {}


def _refs(family):
    """(want, ref32) of a family's case, computed once."""
    if family not in _CACHE:
        make, auto, _, _ = FAMILIES[family]
        case = make()
        _CACHE[family] = (case, auto(case, torch.float64), auto(case, torch.float32))
    return _CACHE[family]


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_float32_restatement_passes_the_bar_and_the_manual_backward_is_the_autograd_one(family):
    case, want, ref32 = _refs(family)
    manual = FAMILIES[family][2]
    exact, m32 = manual(case, torch.float64), manual(case, torch.float32)
    for name in FAMILIES[family][3]:
        assert_bar("%s %s ref32" % (name, family), ref32[name], want[name], ref32[name])
        assert_bar("%s %s manual32" % (name, family), m32[name], want[name], ref32[name])
        scale = float(want[name].abs().max())
        assert float((exact[name] - want[name]).detach().abs().max()) <= 1e-12 * scale, name
        assert scale > 0


def test_the_upstream_scales_put_every_gradient_below_the_old_bar():
    """... so the absolute 1e-4 says nothing about them: that is the gap the bar closes."""
    for family in sorted(FAMILIES):
        _, want, _ = _refs(family)
        for name in FAMILIES[family][3]:
            if name.startswith("d"):
                assert float(want[name].abs().max()) < 1e-4, (family, name)


@pytest.mark.parametrize("family,bug", [("gru", b) for b in GRU_BUGS] + [("addattn", b) for b in ADDATTN_BUGS]
                         + [("capsule", b) for b in CAPSULE_BUGS])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_a_wrong_term_fails_the_bar_and_passes_the_old_absolute_rule(family, bug, dtype):
    case, want, ref32 = _refs(family)
    names = FAMILIES[family][3]
    mutant = FAMILIES[family][2](case, dtype, bug)
    caught = [n for n in names if not within_bar(mutant[n], want[n], ref32[n])]
    for n in names:
        err = float((mutant[n].double() - want[n]).detach().abs().max())
        print("%s / %s / %s: err %.3e scale %.3e %s" % (family, bug, n, err, float(want[n].abs().max()),
                                                        "CAUGHT" if n in caught else "within the bar"))
    assert caught, "%s: '%s' passes the bar on every tensor" % (family, bug)
    assert all(within_absolute(mutant[n], want[n], 1e-4) for n in names), "%s: '%s' is caught by 1e-4 too" % (family, bug)
