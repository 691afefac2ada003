"""Float64 restatements of the interaction and row-scoring kernels that sit behind the embedding lookup in every model
(rbx_interaction.hip: InnerProductInteraction's four modes, rechub FM, fm_sum with the first-order Linear riding in it,
pair_mul; rbx_tower.hip: l2_normalize, pair_dot; rbx_pool.hip: pool), with a bound per element in the conventions of
oracle/fm64.py and oracle/embed64.py:

    |got - want| <= C * eps32 * A + tiny          A: the same sum taken over absolute values

and ``A == 0`` means exactly zero (all-zero rows, F = 1 in the pairwise modes, masked history steps).  Every function
takes float32-representable inputs (they are rounded to float32 first), imports no product code and returns
``(want, A)`` pairs in float64 on the CPU.

Definitions (e [B, F, D]; S = sum_f e, Sa = sum_f |e|, Q = sum_f e^2; pairs p = (i, j), i < j, in triu order):
    bi_interaction   out[b, d] = 0.5 (S^2 - Q)                     A = 0.5 (Sa^2 + Q)
    product_sum      out[b]    = sum_d of the above                A = sum_d of the above      (rechub FM, fm_sum's y_fm)
      gradient       de_f      = g (S - e_f)                       A = |g| (Sa + |e_f|)        g [B, 1] or [B, D]
    inner_product    out[b, p] = <e_i, e_j>                        A = <|e_i|, |e_j|>
      gradient       de_i      = sum_{j != i} g_p e_j              A = sum |g_p| |e_j|
    elementwise_product out[b, p, d] = e_id e_jd                   ONE rounded product: float32(e_i) * float32(e_j)
      gradient       de_id     = sum_{j != i} g_pd e_jd            A = sum |g_pd| |e_jd|
    fm_sum           S [B, D], y_fm (product_sum), y_lr = <x[:, :F D], w> + b        A = Sa; as above; sum |x w| + |b|
    pair_mul         out[b, p, :] = left(b, p) * right[b, j]       left per field ([B, F, D], row i) or per pair ([B, P, D])
      gradients      dright[b, x] = sum_{i < x} g_p left(b, p)     dleft[b, x] = sum_{j > x} g_p right[b, j]   (per field)
                                                                   dleft[b, p] = g_p right[b, j]               (per pair)
    l2_normalize     y = x / max(|x|, eps)                         A = |y|
      gradient       dx = inv (dy - y <y, dy>), plain dy / eps when the clamp was active
                                                                   A = inv (|dy| + |y| sum |y dy|)
    pair_dot         out[b, n] = scale <u_b, v_bn>                 du_b = scale sum_n g_bn v_bn     dv_bn = scale g_bn u_b
    pool             out[b] = inv_b sum_l k_bl e_bl, k = mask when numer_masked else 1; inv_b = 1 / (den_b + eps) with
                     den = 1 (denom 0: inv = 1, eps unused), #{l: sum_d e_bl != 0} (1), sum_l mask (2), L (3)
                                                                   A = inv sum_l |k e|
      gradient       de_bl = k_bl inv_b dout_b                     A = |k inv dout|
    The value count of denom 1 is a knife edge a restatement cannot own: callers keep every row either all zeros or
    with |sum_d e| >= 1e-3 sum_d |e| (``assert_value_rows_are_safe``), so that every float32 summation order agrees.

Constants, from how each kernel sums (never from what it returns); the floor is the project's C_BOUND = 64:
    modes 0 / 1, fm_sum     a lane adds F terms in sequence (S and Q), squares, subtracts, then a tree of at most 6 steps
                            plus NV * 4 register terms: C = max(64, 2 F + 8).  A float32 sequential emulation (randn,
                            one-signed, fields spread over e^+-6; F = 1 .. 4000, D = 2 .. 1000) peaked at 53 x eps32 A
                            (F = 4000, one-signed), 16 at F = 200, 7 at F = 39.
    their gradient          S is F terms in sequence, one subtraction, one product: C = max(64, F + 4)
    inner_product           one lane walks D products: C = max(64, D + 2)
    its and mode 3's gradient, pair_mul's per-field gradients      F - 1 products in sequence: C = max(64, F + 2)
    elementwise_product, pair_mul forward, pair_mul's per-pair dleft   one rounded product: equality (``one_product``)
    pool                    L terms in sequence, one scaling: C = max(64, L + 2); gradient: two products: 64
    l2_normalize, pair_dot  a lane walks ceil(D / G) elements, then a tree: C = max(64, ceil(D / G) + 8),
                            G = min(64, next power of two >= D).  That is the forward (and l2_normalize's <y, dy>).
                            pair_dot's du is N products summed in sequence by one lane, whose own constant would be
                            max(64, N + 2) (103 at N = 101); it is held to the same ceil(D / G) + 8 rule all the same,
                            the tighter of the two there, and dv is two products.
"""
import torch

from oracle.fm64 import C_BOUND, EPS32, TINY, bound_ratio  # noqa: F401  (one set of conventions for the three files)


def _r(x):
    """float32-rounded, then float64, on the CPU."""
    return x.detach().float().double().cpu()


# ---- constants ----------------------------------------------------------------------------------------------------
def lane_group(D):
    g = 1
    while g < D and g < 64:
        g *= 2
    return g


def c_fm_fwd(F):
    return max(C_BOUND, 2 * F + 8)


def c_fm_bwd(F):
    return max(C_BOUND, F + 4)


def c_inner(D):
    return max(C_BOUND, D + 2)


def c_pair_bwd(F):
    return max(C_BOUND, F + 2)


def c_pool(L):
    return max(C_BOUND, L + 2)


def c_rows(D):
    return max(C_BOUND, -(-D // lane_group(D)) + 8)


def one_product(a, b):
    """The float32 product of float32 inputs, as float64: what a kernel that multiplies once must return exactly."""
    return (a.detach().float().cpu() * b.detach().float().cpu()).double()


def ratios(got, want, A, C):
    """|got - want| / (C eps32 A + tiny) per element (float64, shape of want)."""
    got = got.detach().double().cpu().reshape(want.shape)
    return (got - want).abs() / (C * EPS32 * A + TINY)


# ---- modes 0 / 1 ----------------------------------------------------------------------------------------------------
def bi_interaction64(e):
    e = _r(e)
    S, Sa, Q = e.sum(1), e.abs().sum(1), (e * e).sum(1)
    return 0.5 * (S * S - Q), 0.5 * (Sa * Sa + Q)


def product_sum64(e):
    want, A = bi_interaction64(e)
    return want.sum(1, keepdim=True), A.sum(1, keepdim=True)


def fm_grad64(e, g):
    """g: [B, 1] (product_sum) or [B, D] (bi_interaction)."""
    e, g = _r(e), _r(g)
    g = g.reshape(e.shape[0], 1, -1)
    S, Sa = e.sum(1, keepdim=True), e.abs().sum(1, keepdim=True)
    return g * (S - e), g.abs() * (Sa + e.abs())


# ---- modes 2 / 3 ----------------------------------------------------------------------------------------------------
def pairs(F):
    """(i [P], j [P]) of the pairs i < j in triu (row-major) order."""
    idx = torch.triu_indices(F, F, offset=1)
    return idx[0], idx[1]


def inner_product64(e):
    e = _r(e)
    i, j = pairs(e.shape[1])
    return (e[:, i] * e[:, j]).sum(2), (e[:, i] * e[:, j]).abs().sum(2)


def elementwise_product64(e):
    """(want, A) with want the ONE float32 product: compare for equality."""
    i, j = pairs(e.shape[1])
    ef = e.detach().float().cpu()
    want = one_product(ef[:, i], ef[:, j])
    return want, want.abs()


def pair_grad64(e, g):
    """Gradient of inner_product (g [B, P]) or elementwise_product (g [B, P, D])."""
    e, g = _r(e), _r(g)
    B, F, D = e.shape
    i, j = pairs(F)
    want, A = torch.zeros_like(e), torch.zeros_like(e)
    if i.numel() == 0:
        return want, A
    g = g.reshape(B, i.numel(), -1).expand(B, i.numel(), D)
    want.index_add_(1, i, g * e[:, j])
    want.index_add_(1, j, g * e[:, i])
    A.index_add_(1, i, (g * e[:, j]).abs())
    A.index_add_(1, j, (g * e[:, i]).abs())
    return want, A


# ---- fm_sum (DeepFM's input stage) ------------------------------------------------------------------------------------
def fm_sum64(x, F, D, w=None, b=None):
    """x [B, K >= F D].  Returns {"S": (want, A), "y_fm": ..., "y_lr": ...} (y_lr only with w [1, F D] or [F D])."""
    x = _r(x)
    e = x[:, :F * D].reshape(-1, F, D)
    out = {"S": (e.sum(1), e.abs().sum(1)), "y_fm": product_sum64(e)}
    if w is not None:
        t = x[:, :F * D] * _r(w).reshape(1, -1)
        b0 = _r(b).reshape(()) if b is not None else torch.zeros((), dtype=torch.float64)
        out["y_lr"] = (t.sum(1, keepdim=True) + b0, t.abs().sum(1, keepdim=True) + b0.abs())
    return out


# ---- pair_mul -----------------------------------------------------------------------------------------------------------
def pair_mul64(left, right, per_pair):
    """want is the ONE float32 product (equality)."""
    i, j = pairs(right.shape[1])
    lf, rf = left.detach().float().cpu(), right.detach().float().cpu()
    want = one_product(lf if per_pair else lf[:, i], rf[:, j])
    return want, want.abs()


def pair_mul_grad64(left, right, g, per_pair):
    """((dleft, A), (dright, A)); the per-pair dleft is one product (A = |want|, equality with ``one_product``)."""
    left, right, g = _r(left), _r(right), _r(g)
    i, j = pairs(right.shape[1])
    dright, a_right = torch.zeros_like(right), torch.zeros_like(right)
    lp = left if per_pair else left[:, i]
    dright.index_add_(1, j, g * lp)
    a_right.index_add_(1, j, (g * lp).abs())
    if per_pair:
        dleft = one_product(g, right[:, j])
        a_left = dleft.abs()
    else:
        dleft, a_left = torch.zeros_like(left), torch.zeros_like(left)
        dleft.index_add_(1, i, g * right[:, j])
        a_left.index_add_(1, i, (g * right[:, j]).abs())
    return (dleft, a_left), (dright, a_right)


# ---- l2_normalize, pair_dot ---------------------------------------------------------------------------------------------
def l2_normalize64(x, eps=1e-12):
    """(y, A, clamped [rows] bool) over the last axis; eps is the float32 the kernel receives."""
    x = _r(x)
    eps = float(torch.tensor(eps, dtype=torch.float32))
    nrm = (x * x).sum(-1, keepdim=True).sqrt()
    y = x / nrm.clamp_min(eps)
    return y, y.abs(), (nrm < eps).squeeze(-1)


def l2_normalize_grad64(x, dy, eps=1e-12):
    x, dy = _r(x), _r(dy)
    eps = float(torch.tensor(eps, dtype=torch.float32))
    nrm = (x * x).sum(-1, keepdim=True).sqrt()
    inv = 1.0 / nrm.clamp_min(eps)
    y = x * inv
    live = (nrm >= eps).double()
    want = inv * (dy - live * y * (y * dy).sum(-1, keepdim=True))
    A = inv * (dy.abs() + live * y.abs() * (y * dy).abs().sum(-1, keepdim=True))
    return want, A


def pair_dot64(u, v, scale=1.0):
    """u [B, D] or [B, 1, D]; v [B, D] or [B, N, D] -> out [B, N]."""
    u, v = _r(u), _r(v)
    B, D = u.shape[0], u.shape[-1]
    u, v = u.reshape(B, 1, D), v.reshape(B, -1, D)
    s = float(torch.tensor(scale, dtype=torch.float32))
    return s * (u * v).sum(2), abs(s) * (u * v).abs().sum(2)


def pair_dot_grad64(u, v, g, scale=1.0):
    """((du, A), (dv, A)) in the shapes of u and v."""
    ush, vsh = u.shape, v.shape
    u, v, g = _r(u), _r(v), _r(g)
    B, D = u.shape[0], u.shape[-1]
    u, v = u.reshape(B, 1, D), v.reshape(B, -1, D)
    g = g.reshape(B, -1, 1)
    s = float(torch.tensor(scale, dtype=torch.float32))
    du, a_du = s * (g * v).sum(1), abs(s) * (g * v).abs().sum(1)
    dv, a_dv = s * g * u, abs(s) * (g * u).abs()
    return (du.reshape(ush), a_du.reshape(ush)), (dv.reshape(vsh), a_dv.reshape(vsh))


# ---- pool ---------------------------------------------------------------------------------------------------------------
DENOM_NONE, DENOM_VALUE, DENOM_MASK, DENOM_LEN = 0, 1, 2, 3


def _pool_parts(e, mask, numer_masked, denom, eps):
    e = _r(e)
    B, L, _ = e.shape
    m = _r(mask).reshape(B, L) if mask is not None else None
    k = m if numer_masked else torch.ones(B, L, dtype=torch.float64)
    eps = float(torch.tensor(eps, dtype=torch.float32))
    if denom == DENOM_NONE:
        inv = torch.ones(B, dtype=torch.float64)
    else:
        den = {DENOM_VALUE: lambda: (e.sum(2) != 0).double().sum(1), DENOM_MASK: lambda: m.sum(1),
               DENOM_LEN: lambda: torch.full((B,), float(L), dtype=torch.float64)}[denom]()
        inv = 1.0 / (den + eps)
    return e, k, inv


def pool64(e, mask=None, numer_masked=False, denom=DENOM_NONE, eps=0.0):
    e, k, inv = _pool_parts(e, mask, numer_masked, denom, eps)
    t = k[:, :, None] * e
    return inv[:, None] * t.sum(1), inv[:, None] * t.abs().sum(1)


def pool_grad64(e, dout, mask=None, numer_masked=False, denom=DENOM_NONE, eps=0.0):
    e, k, inv = _pool_parts(e, mask, numer_masked, denom, eps)
    want = (k * inv[:, None])[:, :, None] * _r(dout)[:, None, :]
    return want, want.abs()


def assert_value_rows_are_safe(e):
    """denom 1 counts rows whose float32 sum over d is not zero: every row all zeros, or |sum_d e| >= 1e-3 sum_d |e|."""
    e = _r(e)
    s, a = e.sum(-1).abs(), e.abs().sum(-1)
    bad = (a != 0) & (s < 1e-3 * a)
    assert not bool(bad.any()), "%d rows whose sum is within 1e-3 of cancelling" % int(bad.sum())
