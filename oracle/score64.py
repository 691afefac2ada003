"""Float64 restatements of the chain that ends every matching / ranking step: candidate scoring (rbx_gatherdot.hip
gather_dot, rbx_tower.hip cos_dot) and the loss epilogues (rbx_loss.hip softmax_ce and pair_logsigmoid, rbx_tower.hip
bce_mean and the two sigmoid_bce_mean forms), in the conventions of oracle/fm64.py and oracle/interact64.py:

    |got - want| <= C * eps32 * A + tiny          A: the sum of the absolute values of the terms that were added

Plain torch float64 on the CPU; inputs are rounded to float32 first; no product code is imported and nothing here follows
a kernel's summation order.  Every function returns ``(want, A)`` pairs.

Definitions
    gather_dot    out[r, c] = scale <x[r], W_c[id]>                    A = |scale| <|x[r]|, |W_c[id]|>
                  an id outside [0, vocab) scores 0 (A = 0) and has no gradient; the padding row is scored as the row it is
      gradients   dx[r] = scale sum_c g[r, c] W_c[id]                  A = |scale| sum_c |g| |W|
                  dW[id] += scale g[r, c] x[r]  (not for id == padding_idx, not for ids out of range)
    cos_dot       out[b, n] = scale <u_b, v_bn> / max(|v_bn|, eps)     A = |scale| <|u|, |v|> / max(|v|, eps)
      gradients   with a = 1 / max(|v|, eps), vh = a v, c = <u, vh> (c = 0 where the clamp is active: F.normalize's rule)
                  du_b = scale sum_n g vh                              A = |scale| sum_n |g| |vh|
                  dv_bn = scale g a (u - vh c)                         A = |scale g| a (|u| + |vh| <|u|, |vh|>)
                  A zero candidate row scores 0 and adds nothing to du; its dv is scale g u / eps, as autograd's.
    softmax_ce    lse_r = m + log sum_c exp(x_c - m), m = max_c x_c    A_lse = |m| + |log s| + sum_c p_c (1 + |x_c - m|)
                  loss = mean_r (lse_r - x[r, t_r])                    A = mean_r (A_lse + |x_t|)
                  (p = softmax; the sum over c is what one rounding of x_c - m and of a term of s does to log s)
      gradient    dx[r, c] = g / rows (p_c - [c == t])                 A = |g| / rows (p_c (1 + |x_c - lse| + A_lse) + [c == t])
                  a -inf entry away from the target has p = 0 exactly: it adds 0 to the loss and its gradient is 0 (A = 0)
    pair_logsigmoid   loss = scale sum_i -w_i (ls(pos_i) + ls(-neg_i)), ls(v) = min(v, 0) - log1p(exp(-|v|))
                  A = |scale| sum_i |w_i| (|min(pos, 0)| + log1p(e^-|pos|) + the same of -neg);  w_i == 0: never evaluated
      gradients   dpos = -g scale w (1 - sigmoid(pos))                 A = |g scale w| (1 + sigmoid(pos))
                  dneg =  g scale w sigmoid(neg)                       A = |g scale w| sigmoid(neg);  w_i == 0: exactly 0
    bce           mean_i -(y max(log p, -100) + (1 - y) max(log1p(-p), -100))      A = mean (|y| |lp| + |1 - y| |lq|)
      gradient    dp = g / n (p - y) / max((1 - p) p, 1e-12)           A = |dp|   (a subtraction, two products, a division)
    sigmoid_bce   the operation is DEFINED on the float32 probability: p32 = float32(sigmoid(x)); the two clamped log terms
                  and dx = gscale / n (p - y) / max((1 - p) p, 1e-12) (1 - p) p are evaluated in float64 on that p32.
                  Besides A it returns ``cond``, what ONE ulp of p32 does to the result: |y| ulp / p + |1 - y| ulp / (1 - p)
                  for a loss term, ulp gscale / n for dx -- taken as the larger one-sided difference of the float64
                  formula at p32 -+ ulp, so that it stays true where 1 - p is itself one ulp.  That happens at x = 17:
                  float32(sigmoid64(17)) = 1 - 2^-24, while 1 / (1 + expf(-17)) in float32 is 1.0f (1 + 4.1e-8 rounds to
                  1), and on p = 1.0f the term is the clamp's 100 (1 - y) and dx = 0 (sigmoid's backward multiplies by
                  1 - p).  The loss is that sensitive there; a caller that holds the device's own ``prob`` passes it as
                  ``p32=`` and compares without ``cond`` at all.

Constants, from how each kernel sums (never from what it returns); the floor is the project's C_BOUND = 64
    gather_dot forward    a lane sums NV * W <= 16 products in sequence, log2 G <= 6 shuffle adds, one scaling: 23 < 64
    gather_dot dx         n_out products added in sequence (the U-wide candidate loop is unrolled, the order is c), each
                          with the rounded g * scale: C = max(64, 2 n_out + 2)
    gather_dot dW         the sorted segmented reduce of oracle/embed64.py with one more product (scale g): C_BOUND
    cos_dot forward       k = ceil(D / G) elements in sequence (NV * 4 <= 16 in the vector kernels), 6 shuffle adds, for
                          both <u, v> and |v|^2 (half its relative error reaches the norm), sqrt, a division, two
                          products: C = max(64, 3 (k + 6) / 2 + 6)
    cos_dot dv            the saved 1 / |v| enters three times, <u, vh> once: C = max(64, 5 (k + 6) / 2 + 12) (67 at k = 16)
    cos_dot du            N terms in sequence, each with 1 / |v|: C = max(64, N + (k + 6) / 2 + 6)
    loss epilogues        a thread's own elements (softmax: n terms of s and the max; pair / bce: 4 elements in sequence),
                          6 shuffle adds + 4 -> 2 -> 1 adds of the block partial, ceil(blocks / 256) partials per thread in
                          sequence, 6 + 2 adds of the final 256-wide sum, one scaling:
                          C = max(64, per_thread + 18 + ceil(blocks / 256)) + T
    element-wise gradients (softmax dx, pair dpos / dneg, bce dp, sigmoid_bce prob / dx): max(64, ...) + T likewise
T is the allowance for expf / logf / log1pf of the device library, whose accuracy cannot be derived from this repository.
It is MEASURED: the kernels' formulas evaluated element by element in torch float32 on the CPU against this file, on the
inputs of tests/test_gpu_score_forms.py (tests/test_score64_restatement.py::test_float32_formulas_and_the_allowance
recomputes it and fails if 4 x the figure exceeds T):
    softmax lse 0.49, softmax dx 0.49, pair term 1.29, pair gradients 0.98, bce term 0.86, sigmoid prob 1.02,
    sigmoid_bce term 0.98, sigmoid_bce dx 0.60
    (x eps32 A; worst over randn * 4, uniform +-100, constant and masked rows, the ladder -110 .. 110)
T = 6 >= 4 x 1.29 = 5.2: the 4 x is there because the device library may differ from the host's by a few ulp.
"""
import torch

from oracle.fm64 import C_BOUND, EPS32, TINY  # noqa: F401  (one set of conventions)
from oracle.interact64 import lane_group, ratios  # noqa: F401

T_ALLOW = 6
F32_GUARD = float(torch.tensor(1e-12, dtype=torch.float32))


def _r(x):
    """float32-rounded, then float64, on the CPU."""
    return x.detach().float().double().cpu()


def _s(v):
    return float(torch.tensor(v, dtype=torch.float32))


# ---- constants ------------------------------------------------------------------------------------------------------
def _k(D):
    return -(-D // lane_group(D))


def c_dot_fwd(D):
    return C_BOUND


def c_dot_dx(n_out):
    return max(C_BOUND, 2 * n_out + 2)


def c_cos_fwd(D):
    return max(C_BOUND, (3 * (_k(D) + 6)) // 2 + 6)


def c_cos_dv(D):
    return max(C_BOUND, (5 * (_k(D) + 6)) // 2 + 12)


def c_cos_du(D, N):
    return max(C_BOUND, N + (_k(D) + 6) // 2 + 6)


def c_loss(per_thread, blocks):
    return max(C_BOUND, per_thread + 18 + -(-blocks // 256)) + T_ALLOW


def c_elem():
    return C_BOUND + T_ALLOW


# ---- gather_dot -----------------------------------------------------------------------------------------------------
def _rows_of(w, ids):
    """(rows [R, n, D] with zeros for ids outside the table, ok [R, n] bool)."""
    ids = ids.detach().cpu().long().reshape(ids.shape[0], -1)
    ok = (ids >= 0) & (ids < w.shape[0])
    rows = w[ids.clamp(0, w.shape[0] - 1)] * ok[:, :, None].double()
    return rows, ok, ids


def gather_dot(x, tables, id_sets, scale=1.0, padding_idx=None):
    """x [R, D]; tables: one per id set (the same tensor object = a shared table); id_sets: [R] or [R, n_i] each."""
    x, s = _r(x), _s(scale)
    outs, As = [], []
    for w, ids in zip(tables, id_sets):
        rows, _, _ = _rows_of(_r(w), ids)
        t = x[:, None, :] * rows
        outs.append(s * t.sum(2))
        As.append(abs(s) * t.abs().sum(2))
    return torch.cat(outs, 1), torch.cat(As, 1)


def gather_dot_grad(x, tables, id_sets, g, scale=1.0, padding_idx=None):
    """((dx, A), [(dW, A) per DISTINCT table, in order of first use])."""
    x, g, s = _r(x), _r(g), _s(scale)
    dx, a_dx = torch.zeros_like(x), torch.zeros_like(x)
    seen, grads, col = [], [], 0
    for w, ids in zip(tables, id_sets):
        w64 = _r(w)
        rows, ok, ids2 = _rows_of(w64, ids)
        n = ids2.shape[1]
        gc = g[:, col:col + n]
        col += n
        dx += s * (gc[:, :, None] * rows).sum(1)
        a_dx += abs(s) * (gc[:, :, None] * rows).abs().sum(1)
        for k, t in enumerate(seen):
            if t is w:
                break
        else:
            k = len(seen)
            seen.append(w)
            grads.append((torch.zeros_like(w64), torch.zeros_like(w64)))
        live = ok if padding_idx is None else ok & (ids2 != padding_idx)
        contrib = s * (gc * live.double())[:, :, None] * x[:, None, :]
        flat = ids2.clamp(0, w64.shape[0] - 1).reshape(-1)
        grads[k][0].index_add_(0, flat, contrib.reshape(-1, x.shape[1]))
        grads[k][1].index_add_(0, flat, contrib.abs().reshape(-1, x.shape[1]))
    return (dx, a_dx), grads


# ---- cos_dot --------------------------------------------------------------------------------------------------------
def _cos_parts(u, v, eps):
    u, v = _r(u), _r(v)
    B, N, D = v.shape
    u = u.reshape(B, 1, D)
    nrm = (v * v).sum(2, keepdim=True).sqrt()
    a = 1.0 / nrm.clamp_min(_s(eps))
    return u, v, a, (nrm >= _s(eps)).double()


def cos_dot(u, v, eps=1e-12, scale=1.0):
    """u [B, D] (or [B, 1, D]); v [B, N, D] -> out [B, N]."""
    u, v, a, _ = _cos_parts(u, v, eps)
    s = _s(scale)
    return s * (u * v * a).sum(2), abs(s) * (u * v * a).abs().sum(2)


def cos_dot_grad(u, v, g, eps=1e-12, scale=1.0):
    """((du [B, D], A), (dv [B, N, D], A))."""
    u, v, a, live = _cos_parts(u, v, eps)
    B, N, D = v.shape
    g, s = _r(g).reshape(B, N, 1), _s(scale)
    vh = v * a
    c = live * (u * vh).sum(2, keepdim=True)
    ca = live * (u * vh).abs().sum(2, keepdim=True)
    du, a_du = s * (g * vh).sum(1), abs(s) * (g * vh).abs().sum(1)
    dv = s * g * a * (u - vh * c)
    a_dv = (abs(s) * g.abs() * a) * (u.abs() + vh.abs() * ca)
    return (du, a_du), (dv, a_dv)


# ---- softmax cross entropy --------------------------------------------------------------------------------------------
def _softmax_parts(logits, target):
    x = _r(logits)
    rows, n = x.shape
    t = torch.zeros(rows, dtype=torch.long) if target is None else target.detach().cpu().long().reshape(-1)
    m = x.max(1, keepdim=True).values
    d = x - m
    e = d.exp()
    s = e.sum(1, keepdim=True)
    p = e / s
    lse = (m + s.log()).squeeze(1)
    pd = torch.where(p == 0, torch.zeros_like(p), p * (1.0 + d.abs()))
    a_lse = m.abs().squeeze(1) + s.log().abs().squeeze(1) + pd.sum(1)
    return x, t, p, lse, a_lse


def softmax_ce(logits, target=None):
    """((loss, A), (lse [rows], A))."""
    x, t, _, lse, a_lse = _softmax_parts(logits, target)
    xt = x.gather(1, t[:, None]).squeeze(1)
    return ((lse - xt).mean(), (a_lse + xt.abs()).mean()), (lse, a_lse)


def softmax_ce_grad(logits, target=None, g=1.0):
    """(dlogits [rows, n], A) for the upstream gradient g of the scalar loss."""
    x, t, p, lse, a_lse = _softmax_parts(logits, target)
    rows = x.shape[0]
    gs = float(g) / rows
    hot = torch.zeros_like(p).scatter_(1, t[:, None], 1.0)
    dl = (x - lse[:, None]).abs()
    pa = torch.where(p == 0, torch.zeros_like(p), p * (1.0 + dl + a_lse[:, None]))
    return gs * (p - hot), abs(gs) * (pa + hot)


# ---- pairwise log-sigmoid ---------------------------------------------------------------------------------------------
def _ls_parts(v):
    """log sigmoid(v) = lo - sp with lo = min(v, 0), sp = log1p(exp(-|v|)); returns (value, |lo| + sp)."""
    lo, sp = v.clamp_max(0.0), torch.log1p(torch.exp(-v.abs()))
    return lo - sp, lo.abs() + sp


def pair_logsigmoid(pos, neg, w=None, scale=1.0):
    """((loss, A), (terms [n], A [n])): the terms are scale-free, -w (ls(pos) + ls(-neg)), 0 where w == 0."""
    pos, neg = _r(pos).reshape(-1), _r(neg).reshape(-1)
    w = torch.ones_like(pos) if w is None else _r(w).reshape(-1)
    live = w != 0
    zero = torch.zeros_like(pos)
    lp, ap = _ls_parts(torch.where(live, pos, zero))
    ln, an = _ls_parts(torch.where(live, -neg, zero))
    term = torch.where(live, -w * (lp + ln), zero)
    a = torch.where(live, w.abs() * (ap + an), zero)
    s = _s(scale)
    return (s * term.sum(), abs(s) * a.sum()), (term, a)


def pair_logsigmoid_grad(pos, neg, w=None, scale=1.0, g=1.0):
    """((dpos, A), (dneg, A)); exactly 0 (A = 0) where w == 0, whatever the position holds."""
    pos, neg = _r(pos).reshape(-1), _r(neg).reshape(-1)
    w = torch.ones_like(pos) if w is None else _r(w).reshape(-1)
    live = w != 0
    zero = torch.zeros_like(pos)
    gw = float(g) * _s(scale) * w
    sp = torch.sigmoid(torch.where(live, pos, zero))
    sn = torch.sigmoid(torch.where(live, neg, zero))
    # 1 - sigmoid(v) = sigmoid(-v), without the cancellation
    dpos = torch.where(live, -gw * torch.sigmoid(torch.where(live, -pos, zero)), zero)
    dneg = torch.where(live, gw * sn, zero)
    return (dpos, torch.where(live, gw.abs() * (1.0 + sp), zero)), (dneg, torch.where(live, gw.abs() * sn, zero))


# ---- BCE on probabilities -----------------------------------------------------------------------------------------------
def _bce_parts(p, y):
    """The y part and the 1 - y part of a term."""
    return -y * torch.log(p).clamp_min(-100.0), -(1.0 - y) * torch.log1p(-p).clamp_min(-100.0)


def _bce_terms(p, y):
    a, b = _bce_parts(p, y)
    return a + b, a.abs() + b.abs()


def bce(p, y):
    """((loss, A), (terms [n], A [n])) with torch's clamp of both log terms at -100."""
    p, y = _r(p).reshape(-1), _r(y).reshape(-1)
    term, a = _bce_terms(p, y)
    return (term.mean(), a.mean()), (term, a)


def bce_grad(p, y, g=1.0):
    """(dp, A): g / n (p - y) / max((1 - p) p, 1e-12f)."""
    p, y = _r(p).reshape(-1), _r(y).reshape(-1)
    dp = float(g) / p.numel() * (p - y) / ((1.0 - p) * p).clamp_min(F32_GUARD)
    return dp, dp.abs()


# ---- sigmoid + BCE ------------------------------------------------------------------------------------------------------
def sigmoid32(x):
    """float32(sigmoid64(x)) as float64: the probability the operation is defined on."""
    return torch.sigmoid(_r(x).reshape(-1)).float().double()


def _ulp32(p32):
    """The spacing of float32 at p32 (the smaller of the two neighbours' distances), float64."""
    f = p32.float()
    up = torch.nextafter(f, torch.full_like(f, 2.0)).double() - p32
    dn = p32 - torch.nextafter(f, torch.full_like(f, -1.0)).double()
    return torch.minimum(up, dn)


def _sb_dx(p, y, gs):
    q = (1.0 - p) * p
    return gs * (p - y) / q.clamp_min(F32_GUARD) * q


def sigmoid_bce(x, y, grad_scale=1.0, p32=None):
    """{"prob": (p32, A), "loss": (loss, A, cond), "terms": (terms, A, cond), "dx": (dx, A, cond)}.
    p32: the float32 probabilities to evaluate on (default: float32(sigmoid64(x))); cond: see the module docstring."""
    y = _r(y).reshape(-1)
    p = sigmoid32(x) if p32 is None else _r(p32).reshape(-1)
    n = p.numel()
    gs = _s(grad_scale) / n
    term, a = _bce_terms(p, y)
    dx = _sb_dx(p, y, gs)
    ulp = _ulp32(p)
    lo, hi = (p - ulp).clamp_min(0.0), (p + ulp).clamp_max(1.0)
    parts = _bce_parts(p, y)
    c_term = sum(torch.maximum((l - m).abs(), (h - m).abs()) for l, m, h in zip(_bce_parts(lo, y), parts, _bce_parts(hi, y)))
    c_dx = torch.maximum((_sb_dx(lo, y, gs) - dx).abs(), (_sb_dx(hi, y, gs) - dx).abs())
    return {"prob": (p, p.abs()), "terms": (term, a, c_term), "loss": (term.mean(), a.mean(), c_term.mean()),
            "dx": (dx, dx.abs() + abs(gs) * (p + y.abs()), c_dx)}
