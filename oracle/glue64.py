"""Float64 restatements of the streaming "glue" kernels at the end of rbx_tower.hip (cross_fwd / cross_bwd, rowscale,
rowscale_seq, seq_colsum, sum_prefix, scale_by_scalar) and of rbx_cin.hip (cin_outer_fwd / cin_outer_bwd), in the conventions
of oracle/fm64.py:

    |got - want| <= C * eps32 * A + tiny          A: the sum of the absolute values of the terms that were added

Plain torch float64 on the CPU; inputs are rounded to float32 first; no product code is imported, nothing here uses
autograd (the backward formulas are written out) and nothing follows a kernel's summation order.  Every function returns
``(want, A)`` pairs.  A result that is ONE product of two float32 values is exact in float64 (48 significant bits), so
``want.float()`` is the correctly rounded float32 result and such outputs are compared for equality, not against a bound.

Definitions
    cross forward     out = xi + x0 h + bias       h [rows, dim], or [rows, 1] broadcast over the row; bias [dim] or None
                      A = |xi| + |x0 h| + |bias|
    cross backward    dx0 = g h, dh = g x0 (h_cols == dim): one product each -> equality
                      dh[r] = sum_c g[r, c] x0[r, c] (h_cols == 1)         A = sum_c |g x0|
    rowscale          out[r, :] = (alpha x[r, :] + add[r, :]) s[r]          A = (|alpha x| + |add|) |s|
                      without add and with alpha == 1 it is the one product x s -> equality
    rowscale_seq      the same with add[r] = pos[r % L]: x [B, L, D], pos [L, D], s [B, L]
    seq_colsum        out[l, :] = sum_b s[b, l] g[b, l, :]                  A = sum_b |s g|     (batch == 0: exactly zero)
    sum_prefix        out[r, c] = base[r, c] + (c < prefix ? a[r, c] + b[r, c] : 0), c < cols   A = |base| + |a| + |b|
                      one operand present: a copy -> equality; none: exactly zero
    scale_by_scalar   y = scalar x: one product -> equality
    cin forward       z[(b, d), h M + m] = x0[b, h, d] xk[(b, d), m]  (xk None: xk[(b, d), m] = x0[b, m, d]) -> equality
    cin backward      dxk[(b, d), m] = sum_h dz[(b, d), h M + m] x0[b, h, d]
                      dx0[b, h, d]   = sum_m dz[(b, d), h M + m] xk[(b, d), m]
                                       (+ sum_h' dz[(b, d), h' M + h] x0[b, h', d] when X_k = X_0)
                      A: the same sums over absolute products

Constants, from how each kernel sums (never from what it returns); the floor is the project's C_BOUND = 64
    cross forward     b + (a h + bias): a product, two additions (or one fused multiply-add and one addition), each
                      rounding at most eps32 / 2 of a partial result that A bounds: 3 roundings, 1.5 eps32 A.  C_BOUND.
    cross dh, row sum lane c % 64 of the 64-lane group adds its ceil(dim / 64) products in sequence, then the six butterfly
                      steps of group_sum<64>: depth = ceil(dim / 64) + 6, one more rounding for each product:
                      C = max(64, depth + 2)
    rowscale (_seq)   (alpha x + add) s: three roundings on A.  C_BOUND.
    seq_colsum        a block partial adds up to 32 products s g in ascending order of b (8 in flight, added in order; the
                      clamped rows of a ragged last trip enter with s = 0 and add exact zeros), the final kernel adds the
                      nb = ceil(batch / 32) partials in ascending order: depth = min(batch, 32) + nb,
                      C = max(64, depth + 2)
    sum_prefix        (base + a) + b: two roundings on A.  C_BOUND.
    cin dxk           F products added in sequence: C = max(64, F + 2)
    cin dx0           M products in sequence; when X_k = X_0, F more in a sum of their own and one addition of the two:
                      terms = M (+ F + 1), C = max(64, terms + 2)
For a sequential float32 sum of n terms the error is at most (n - 1) eps32 / 2 times the sum of absolute values, plus
eps32 / 2 per product; depth + 2 is twice that, so the CPU evaluation of the same orders
(tests/test_glue64_restatement.py) has to stay below 0.5 of every bound.
"""
import torch

from oracle.fm64 import C_BOUND, EPS32, TINY, bound_ratio  # noqa: F401  (one set of conventions)

SEQ_SUM_ROWS = 32               # sequences per block partial of seq_colsum
CROSS_GROUP = 64                # lanes that walk one row in cross_bwd


def _r(x):
    """float32-rounded, then float64, on the CPU."""
    return x.detach().float().double().cpu()


def _s(v):
    return float(torch.tensor(v, dtype=torch.float32))


# ---- constants ------------------------------------------------------------------------------------------------------
def c_cross_fwd():
    return C_BOUND


def c_cross_dh(dim):
    return max(C_BOUND, -(-dim // CROSS_GROUP) + 6 + 2)


def c_rowscale():
    return C_BOUND


def c_colsum(batch):
    nb = -(-batch // SEQ_SUM_ROWS)
    return max(C_BOUND, min(batch, SEQ_SUM_ROWS) + nb + 2)


def c_sum_prefix():
    return C_BOUND


def c_cin_dxk(F):
    return max(C_BOUND, F + 2)


def c_cin_dx0(F, M, own):
    return max(C_BOUND, M + (F + 1 if own else 0) + 2)


# ---- cross ----------------------------------------------------------------------------------------------------------
def cross_fwd(x0, xi, h, bias=None):
    """x0, xi [rows, dim]; h [rows, dim] or [rows, 1]; bias [dim] or None."""
    x0, xi, h = _r(x0), _r(xi), _r(h)
    p = x0 * h
    want, A = xi + p, xi.abs() + p.abs()
    if bias is not None:
        b = _r(bias).view(1, -1)
        want, A = want + b, A + b.abs()
    return want, A


def cross_bwd(x0, h, g):
    """((dx0, A), (dh, A)); dh is [rows, 1] when h is."""
    x0, h, g = _r(x0), _r(h), _r(g)
    dx0 = g * h
    t = g * x0
    if h.shape[1] == 1:
        return (dx0, dx0.abs()), (t.sum(1, keepdim=True), t.abs().sum(1, keepdim=True))
    return (dx0, dx0.abs()), (t, t.abs())


# ---- rowscale -------------------------------------------------------------------------------------------------------
def rowscale(x, add, s, alpha=1.0):
    """x [..., D], add like x or None, s with one value per row of x."""
    x, al = _r(x), _s(alpha)
    s = _r(s).reshape(x.shape[:-1] + (1,))
    t = al * x
    A = t.abs()
    if add is not None:
        a = _r(add)
        t, A = t + a, A + a.abs()
    return t * s, A * s.abs()


def rowscale_seq(x, pos, keep, alpha=1.0):
    """x [B, L, D], pos [L, D], keep [B, L]."""
    return rowscale(x, _r(pos).unsqueeze(0).expand(x.shape), keep, alpha)


def seq_colsum(g, s):
    """g [B, L, D], s [B, L] -> [L, D]."""
    t = _r(g) * _r(s).unsqueeze(-1)
    return t.sum(0), t.abs().sum(0)


def sasrec_input_bwd(g, keep, alpha=1.0):
    """The gradients of (alpha e + pos[None]) keep[..., None] for an upstream g: ((de, A), (dpos, A))."""
    return rowscale(g, None, keep, alpha), seq_colsum(g, keep)


# ---- sum_prefix -----------------------------------------------------------------------------------------------------
def sum_prefix(base, a, b, rows, cols, prefix):
    """base [rows, >= cols], a / b [rows, >= prefix] or None (their further columns are not looked at)."""
    want = torch.zeros(rows, cols, dtype=torch.float64)
    A = torch.zeros_like(want)
    if base is not None:
        t = _r(base)[:, :cols]
        want, A = want + t, A + t.abs()
    for t in (a, b):
        if t is not None and prefix > 0:
            t = _r(t)[:, :prefix]
            want[:, :prefix] += t
            A[:, :prefix] += t.abs()
    return want, A


def scale_by_scalar(x, scalar):
    t = _r(x) * _r(scalar).reshape(())
    return t, t.abs()


# ---- CIN ------------------------------------------------------------------------------------------------------------
def _cin_operands(x0, xk):
    x0 = _r(x0)                                            # [B, F, D]
    B, F, D = x0.shape
    k = x0.transpose(1, 2) if xk is None else _r(xk).view(B, D, -1)          # [B, D, M]
    return x0, k


def cin_fwd(x0, xk=None):
    """z [(b, d), h M + m]."""
    x0, k = _cin_operands(x0, xk)
    B, F, D = x0.shape
    z = x0.permute(0, 2, 1).unsqueeze(3) * k.unsqueeze(2)                    # [B, D, F, M]
    z = z.reshape(B * D, F * k.shape[2])
    return z, z.abs()


def cin_bwd(x0, xk, dz):
    """((dx0, A), (dxk, A) or None when X_k = X_0)."""
    x0, k = _cin_operands(x0, xk)
    B, F, D = x0.shape
    M = k.shape[2]
    g = _r(dz).view(B, D, F, M)
    x0t = x0.permute(0, 2, 1)                                                # [B, D, F]

    def both(gg, kk, xx):
        d0 = (gg * kk.unsqueeze(2)).sum(3)                                   # [B, D, F]: over m
        dk = (gg * xx.unsqueeze(3)).sum(2)                                   # [B, D, M]: over h
        return d0, dk

    d0, dk = both(g, k, x0t)
    a0, ak = both(g.abs(), k.abs(), x0t.abs())
    if xk is None:
        d0, a0 = d0 + dk, a0 + ak
        return (d0.permute(0, 2, 1).contiguous(), a0.permute(0, 2, 1).contiguous()), None
    return (d0.permute(0, 2, 1).contiguous(), a0.permute(0, 2, 1).contiguous()), (dk.reshape(B * D, M), ak.reshape(B * D, M))
