"""Float64 restatements of the normalisation family (rbx_norm.hip: BatchNorm forward / backward / evaluation, its ReLU and
PReLU fused variants, the split entry points behind SyncBatchNorm, LayerNorm; rbx_act.hip: Dice and the stand-alone
PReLU), with a bound per element in the conventions of oracle/fm64.py and oracle/interact64.py:

    |got - want| <= C * eps32 * A + tiny

``A == 0`` means exactly zero.  Every function rounds its inputs to float32 first, imports no product code, uses no
autograd and returns ``(want, A)`` pairs in float64 on the CPU.

Magnitudes.  A normalised value is a difference of two numbers that may be large: xhat = (x - mean) rstd is computed from
x and mean as they are, so its rounding scales with Axh = (|x| + |mean|) rstd, not with |xhat|.  Every A below is the
expression with Axh in the place of |xhat| and absolute values elsewhere -- a mean far from zero is then a fair input:
the bound grows with |mean| rstd exactly as the rounding of x - mean does, and no faster.
    statistics      mean: A = mean |x|            M2 = sum (x - mean)^2: A = sum (|x| + |mean|)^2
                    rstd = 1 / sqrt(M2 / n + eps): A = rstd (1 + 0.5 (A_M2 / n) / (var + eps))   (relative error of var + eps)
    running stats   r' = (1 - m) r + m s: A = |1 - m| A_r + m A_s (A_r carried from step to step), s = mean or M2 / (n - 1);
                    momentum None = cumulative average, m = 1 / num_batches_tracked
    BatchNorm / LayerNorm forward     z = xhat gamma + beta: A_z = Axh |gamma| + |beta|;  ReLU: A = A_z where z > 0, else 0;
                    PReLU: A = A_z where z > 0, else |slope| A_z (z > 0 ? 1 : slope -- z == 0 takes the slope side)
    column sums     dbeta = sum g: A = sum |g|;  dgamma = sum g xhat: A = sum |g| Axh;  dslope = sum_{z <= 0} dy z:
                    A = sum |dy| A_z;  g = dy, masked by the ReLU, or scaled by the PReLU
    dx (BatchNorm)  gamma rstd (g - dbeta / M - xhat dgamma / M): A = |gamma| rstd (|g| + A_dbeta / M + Axh A_dgamma / M)
    dx (LayerNorm)  rstd (g - mean_d g - xhat mean_d (g xhat)), g = dy gamma: the same with means over the row
    Dice            p = sigmoid(xhat), y = x (p + alpha (1 - p)).  An error dt of xhat moves p by p (1 - p) dt, and 1 - p
                    is a float32 subtraction from a rounded p: its error is u (p + (1 - p)), so its magnitude is 1, not
                    1 - p (evaluation mode on far-from-zero inputs has xhat in the thousands and 1 - p below eps32):
                    A_y = |x| (p + |alpha| + |1 - alpha| p (1 - p) Axh)
                    dxhat = dy x (1 - alpha) p (1 - p): A_dxhat = |dy x (1 - alpha)| p (1 + (1 - p) Axh)
                    s1 = sum dxhat: A = sum A_dxhat;  s2 = sum dxhat xhat: A = 2 sum A_dxhat Axh
                    dalpha = sum dy (1 - p) x: A = sum |dy x| (1 + p (1 - p) Axh)
                    dx = dy (p + alpha (1 - p)) + rstd (dxhat - s1 / n - xhat s2 / n)     (evaluation: + rstd dxhat)
                    A = |dy| A_y / |x| + rstd (A_dxhat + A_s1 / n + Axh A_s2 / n)
    PReLU           y = x > 0 ? x : a x and dx = x > 0 ? dy : a dy are ONE rounded product: equality;
                    dslope = sum_{x <= 0} dy x: A = sum |dy x|

Constants, from how each kernel sums (never from what it returns).  One rounding is u = eps32 / 2; the floor is the
project's C_BOUND = 64.  ``depth`` is the number of dependent additions on the longest path of a reduction in the kernel's
fixed order, not the number of terms:
    bn_depth(rows)  bn_stats_partial_kernel: a lane folds ceil(min(rows, R) / 4) rows (R = 64 rows per block below 32 768
                    rows, 256 from there on), <= 3 Chan merges of the row lanes; bn_stats_final_kernel: a wavefront merges
                    ceil(nb / 16) blocks in sequence, <= 15 merges of the wavefronts.  (Merging an empty partial is exact.)
    c_bn_mean = max(64, depth + 8)      a Welford step rounds mean + d / n once at |mean| and d / n twice: <= 2 u A a step
    c_bn_m2   = max(64, 4 depth)        a step rounds d, x - mean', their product and the sum (2 eps32 of the running M2) and
                    carries the mean's error as 2 dmean sum |x - mean| <= depth eps32 A_M2 (Chan, Golub, LeVeque 1983)
    c_bn_stat = 6 depth                 what the statistics' error adds to anything computed from xhat: dmean rstd
                    (depth / 2) and rstd's relative error r times |xhat|, r <= dmean rstd mean|xhat| + 2 depth eps32 -- the
                    first-order term, M2's own roundings being relative to M2: together depth (0.5 (1 + |xhat|) + 2) eps32
                    Axh, which is 6 depth up to |xhat| = 7
    c_bn_y    = 64 + c_bn_stat(rows)    (the element-wise part is a subtraction, three products and an addition: the floor);
                    with the kernel's own mean / rstd handed to the restatement (evaluation mode, the C entry points) it is 64
    c_bn_sum  = max(64, sum depth)      bn_bwd_partial_kernel: a lane adds ceil(min(rows, R) / 4) terms, a tree of 2;
                    bn_bwd_final_kernel: a wavefront adds ceil(nb / 4) partials, a tree of 2.  dbeta.
    dgamma, dslope  c_bn_sum + c_bn_stat + 8 (their terms hold xhat, and its own roundings);   dx: c_bn_sum + 2 c_bn_stat + 64 (dgamma's error, xhat's
                    own, rstd's, the element-wise part)
    LayerNorm       ln_depth(dim) = NV W + log2 G (a lane adds its NV W slots, then a butterfly over the G lanes);
                    two-pass: mean c = 64, c_ln_stat = 6 ln_depth (the variance's first-order term in dmean vanishes; the
                    same allowance is kept), c_ln_y = 64 + c_ln_stat, rstd 64 + c_ln_stat on the A above.
                    dgamma / dbeta: ln_sum_depth -- fused with dx: a lane group adds ceil(rows / groups) rows, the 256 / G
                    groups of a workgroup in sequence, then bn_bwd_final_kernel over the workgroups; parameter gradients
                    only: 256 rows a lane, a tree of 2, the final kernel over blocks of 1024 rows.
                    dx: 64 + 2 c_ln_stat (two row means of ln_depth each are inside c_ln_stat's 6)
    Dice            act_depth(rows): a lane folds min(rows, 256) / 4 rows, 3 merges, then ALL blocks in sequence
                    (dice_stats_final_kernel is one lane per column); the sums likewise.  c_dice_y = 64 + 6 act_depth,
                    c_dice_bwd = 64 + 12 act_depth + sum depth; evaluation mode keeps the same constants (the statistics are
                    then inputs, the allowance is simply not used).  rsqrtf and expf are within 2 ulp: inside the floor.
    PReLU dslope    a lane adds min(rows, 256) / 4 terms, a tree of 2, colsum_final_kernel adds the blocks in sequence; one
                    slope for all columns: a lane adds ceil(cols / 256) columns' blocks in sequence, then a tree of 8.
Row counts above 2^24 are out of scope: the Welford count is a float and stops being exact there.
"""
import torch

from oracle.fm64 import C_BOUND, EPS32, TINY  # noqa: F401
from oracle.interact64 import ratios  # noqa: F401  (the one criterion of the three files)


def _r(x):
    """float32-rounded, then float64, on the CPU."""
    return x.detach().float().double().cpu()


def _d(x):
    """A statistic handed over: float64 as it is (a float32 tensor from a kernel converts exactly)."""
    return x.detach().double().cpu()


def f32(v):
    return float(torch.tensor(float(v), dtype=torch.float32))


def _opt(t, cols, fill):
    return torch.full((cols,), fill, dtype=torch.float64) if t is None else _r(t).reshape(-1)


# ---- constants ----------------------------------------------------------------------------------------------------
def _ceil(a, b):
    return -(-a // b)


def bn_rows_per_block(rows):
    return 256 if rows >= 32768 else 64


def bn_depth(rows):
    rpb = bn_rows_per_block(rows)
    nb = _ceil(rows, rpb)
    return _ceil(min(rows, rpb), 4) + min(3, max(0, min(rows, rpb) - 1)) + _ceil(nb, 16) + min(15, nb - 1)


def c_bn_mean(rows):
    return max(C_BOUND, bn_depth(rows) + 8)


def c_bn_m2(rows):
    return max(C_BOUND, 4 * bn_depth(rows))


def c_bn_stat(rows):
    """rows None: the statistics are inputs (evaluation mode, or the kernel's own mean / rstd handed over)."""
    return 0 if rows is None else 6 * bn_depth(rows)


def c_bn_y(rows):
    return C_BOUND + c_bn_stat(rows)


def bn_sum_depth(rows):
    rpb = bn_rows_per_block(rows)
    return _ceil(min(rows, rpb), 4) + 2 + _ceil(_ceil(rows, rpb), 4) + 2


def c_bn_sum(rows):
    return max(C_BOUND, bn_sum_depth(rows))


def c_bn_dgamma(rows, stat_rows):
    return c_bn_sum(rows) + c_bn_stat(stat_rows) + 8


def c_bn_dx(rows, stat_rows):
    return c_bn_sum(rows) + 2 * c_bn_stat(stat_rows) + C_BOUND


def ln_form(dim, vec=None):
    """(G, NV, vec) of ln_fwd_kernel / ln_bwd_dx_kernel, or None where rbx_layernorm_* refuses the dim."""
    vec = (dim % 4 == 0) if vec is None else vec
    units = dim // 4 if vec else dim
    p = 1
    while p < units:
        p *= 2
    if p > 256:
        return None
    return (min(p, 64), max(1, p // 64), vec)


def ln_depth(dim, vec=None):
    G, NV, vec = ln_form(dim, vec)
    return NV * (4 if vec else 1) + G.bit_length() - 1


def c_ln_stat(dim, vec=None):
    return 6 * ln_depth(dim, vec)


def c_ln_y(dim, vec=None):
    return C_BOUND + c_ln_stat(dim, vec)


def c_ln_dx(dim, vec=None):
    return C_BOUND + 2 * c_ln_stat(dim, vec)


def ln_sum_depth(rows, dim, fused, vec=None, cus=256):
    if not fused:
        nb = _ceil(rows, 1024)
        return _ceil(min(rows, 1024), 4) + 2 + _ceil(nb, 4) + 2
    G = ln_form(dim, vec)[0]
    gpb = 256 // G
    blocks = min(_ceil(rows, gpb), 4 * cus)
    return _ceil(rows, blocks * gpb) + gpb + _ceil(blocks, 4) + 2


def c_ln_sum(rows, dim, fused, vec=None):
    return max(C_BOUND, ln_sum_depth(rows, dim, fused, vec))


def act_depth(rows):
    return _ceil(min(rows, 256), 4) + 3 + _ceil(rows, 256)


def c_dice_y(rows):
    return C_BOUND + 6 * act_depth(rows)


def c_dice_bwd(rows):
    return C_BOUND + 12 * act_depth(rows) + act_depth(rows)


def c_prelu_dslope(rows, cols, n_slope):
    nb = _ceil(rows, 256)
    d = _ceil(min(rows, 256), 4) + 2 + (nb if n_slope != 1 else nb * _ceil(cols, 256) + 8)
    return max(C_BOUND, d)


# ---- BatchNorm ------------------------------------------------------------------------------------------------------
def bn_stats64(x, eps=1e-5):
    """Per column over the rows of x [rows, cols]: {"n", "mean": (want, A), "m2": (want, A), "var", "unbiased",
    "rstd": (want, A)}; var is the biased one (what normalises), unbiased falls back to it with one row."""
    x = _r(x)
    n = x.shape[0]
    eps = f32(eps)
    mean = x.mean(0)
    m2 = ((x - mean) ** 2).sum(0)
    a_m2 = ((x.abs() + mean.abs()) ** 2).sum(0)
    var = m2 / n
    rstd = 1.0 / torch.sqrt(var + eps)
    return {"n": n, "mean": (mean, x.abs().mean(0)), "m2": (m2, a_m2), "var": var,
            "unbiased": m2 / (n - 1) if n > 1 else var,
            "rstd": (rstd, rstd * (1.0 + 0.5 * (a_m2 / n) / (var + eps)))}


def bn_running64(stats, running_mean, running_var, momentum, num_batches_tracked=0):
    """One training step's update.  running_mean / running_var: (value, A) pairs (A = |value| for a fresh buffer).
    momentum None: the cumulative average 1 / (num_batches_tracked + 1).  Returns ((mean', A), (var', A), tracked + 1)."""
    nbt = num_batches_tracked + 1
    m = f32(1.0 / nbt if momentum is None else momentum)
    n = stats["n"]
    (rm, a_rm), (rv, a_rv) = running_mean, running_var
    a_unb = stats["m2"][1] / (n - 1 if n > 1 else n)
    return ((1 - m) * rm + m * stats["mean"][0], abs(1 - m) * a_rm + m * stats["mean"][1]), \
           ((1 - m) * rv + m * stats["unbiased"], abs(1 - m) * a_rv + m * a_unb), nbt


def _slope_of(slope, cols):
    s = _r(slope).reshape(-1)
    return s.expand(cols) if s.numel() == 1 else s


def bn_fwd64(x, gamma, beta, eps=1e-5, relu=False, slope=None, mean=None, rstd=None):
    """z = (x - mean) rstd gamma + beta, then ReLU or PReLU (slope: 1 or cols values).  mean / rstd None: the batch's own
    (training).  Returns {"y": (want, A), "z": (z, A_z), "mean", "rstd"}."""
    x = _r(x)
    cols = x.shape[1]
    if mean is None:
        st = bn_stats64(x, eps)
        mean, rstd = st["mean"][0], st["rstd"][0]
    else:
        mean, rstd = _d(mean), _d(rstd)
    g, b = _opt(gamma, cols, 1.0), _opt(beta, cols, 0.0)
    z = (x - mean) * rstd * g + b
    a_z = (x.abs() + mean.abs()) * rstd * g.abs() + b.abs()
    y, A = z, a_z
    if relu:
        y, A = z.clamp_min(0.0), torch.where(z > 0, a_z, torch.zeros_like(a_z))
    if slope is not None:
        s = _slope_of(slope, cols)
        y, A = torch.where(z > 0, y, s * y), torch.where(z > 0, A, s.abs() * A)
    return {"y": (y, A), "z": (z, a_z), "mean": mean, "rstd": rstd}


def bn_bwd64(x, dy, gamma, mean, rstd, training, total_rows=None, relu_mask=None, slope=None, beta=None, sums=None):
    """The gradients for given mean / rstd.  relu_mask: bool [rows, cols] (y > 0) of a fused ReLU; slope (+ beta): PReLU
    behind the normalisation.  total_rows / sums: a chunk of a larger batch (the split entry points): dx then uses
    sums = ((dbeta, A), (dgamma, A)) of the whole batch and M = total_rows.
    Returns {"dbeta", "dgamma", "dslope" (per column, PReLU only), "dx"}: (want, A) each."""
    x, dy, mean, rstd = _r(x), _r(dy), _d(mean), _d(rstd)
    rows, cols = x.shape
    g_ = _opt(gamma, cols, 1.0)
    xhat = (x - mean) * rstd
    axh = (x.abs() + mean.abs()) * rstd
    g = dy
    out = {}
    if relu_mask is not None:
        g = torch.where(relu_mask.cpu(), dy, torch.zeros_like(dy))
    if slope is not None:
        s, b = _slope_of(slope, cols), _opt(beta, cols, 0.0)
        z, a_z = xhat * g_ + b, axh * g_.abs() + b.abs()
        pos = z > 0
        g = torch.where(pos, dy, s * dy)
        zero = torch.zeros_like(dy)
        out["dslope"] = (torch.where(pos, zero, dy * z).sum(0), torch.where(pos, zero, dy.abs() * a_z).sum(0))
    out["dbeta"] = (g.sum(0), g.abs().sum(0))
    out["dgamma"] = ((g * xhat).sum(0), (g.abs() * axh).sum(0))
    if training:
        (db, a_db), (dg, a_dg) = sums if sums is not None else (out["dbeta"], out["dgamma"])
        M = float(total_rows if total_rows is not None else rows)
        out["dx"] = (g_ * rstd * (g - db / M - xhat * dg / M), g_.abs() * rstd * (g.abs() + a_db / M + axh * a_dg / M))
    else:
        out["dx"] = (g_ * rstd * g, (g_ * rstd * g).abs())
    return out


# ---- LayerNorm ------------------------------------------------------------------------------------------------------
def ln_fwd64(x, gamma, beta, eps=1e-5):
    """x [rows, dim].  {"mean": (want, A), "rstd": (want, A), "y": (want, A)}."""
    x = _r(x)
    dim = x.shape[1]
    eps = f32(eps)
    mean = x.mean(1, keepdim=True)
    var = ((x - mean) ** 2).mean(1, keepdim=True)
    a_var = ((x.abs() + mean.abs()) ** 2).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    g, b = _opt(gamma, dim, 1.0), _opt(beta, dim, 0.0)
    y = (x - mean) * rstd * g + b
    A = (x.abs() + mean.abs()) * rstd * g.abs() + b.abs()
    return {"mean": (mean.squeeze(1), x.abs().mean(1)),
            "rstd": (rstd.squeeze(1), (rstd * (1.0 + 0.5 * a_var / (var + eps))).squeeze(1)), "y": (y, A)}


def ln_bwd64(x, dy, gamma, eps=1e-5, mean=None, rstd=None):
    """{"dx", "dgamma", "dbeta"}: (want, A) each; mean / rstd [rows] None: the rows' own."""
    x, dy = _r(x), _r(dy)
    dim = x.shape[1]
    if mean is None:
        st = ln_fwd64(x, None, None, eps)
        mean, rstd = st["mean"][0], st["rstd"][0]
    mean, rstd = _d(mean).reshape(-1, 1), _d(rstd).reshape(-1, 1)
    gm = _opt(gamma, dim, 1.0)
    xhat = (x - mean) * rstd
    axh = (x.abs() + mean.abs()) * rstd
    g = dy * gm
    m1, m2 = g.mean(1, keepdim=True), (g * xhat).mean(1, keepdim=True)
    a1, a2 = g.abs().mean(1, keepdim=True), (g.abs() * axh).mean(1, keepdim=True)
    return {"dx": (rstd * (g - m1 - xhat * m2), rstd * (g.abs() + a1 + axh * a2)),
            "dgamma": ((dy * xhat).sum(0), (dy.abs() * axh).sum(0)), "dbeta": (dy.sum(0), dy.abs().sum(0))}


# ---- Dice ---------------------------------------------------------------------------------------------------------------
def _dice_parts(x, alpha, eps, mean, rstd):
    x = _r(x)
    if mean is None:
        st = bn_stats64(x, eps)
        mean, rstd = st["mean"][0], st["rstd"][0]
    else:
        mean, rstd = _d(mean), _d(rstd)
    al = _r(alpha).reshape(-1)
    xhat = (x - mean) * rstd
    axh = (x.abs() + mean.abs()) * rstd
    p = torch.sigmoid(xhat)
    return x, al, rstd, xhat, axh, p


def dice_fwd64(x, alpha, eps=1e-9, mean=None, rstd=None):
    x, al, rstd, xhat, axh, p = _dice_parts(x, alpha, eps, mean, rstd)
    q = 1 - p
    return x * (p + al * q), x.abs() * (p + al.abs() + (1 - al).abs() * p * q * axh)


def dice_bwd64(x, dy, alpha, mean, rstd, training, eps=1e-9):
    """{"dalpha", "dx"}: (want, A) each, for given (or, None, the batch's own) mean / rstd."""
    x, al, rstd, xhat, axh, p = _dice_parts(x, alpha, eps, mean, rstd)
    dy = _r(dy)
    n = float(x.shape[0])
    q = 1 - p
    dxh = dy * x * (1 - al) * p * q
    a_dxh = (dy * x * (1 - al)).abs() * p * (1 + q * axh)
    gate, a_gate = p + al * q, p + al.abs() + (1 - al).abs() * p * q * axh
    t, a_t = dxh, a_dxh
    if training:
        s1, a_s1 = dxh.sum(0), a_dxh.sum(0)
        s2, a_s2 = (dxh * xhat).sum(0), 2 * (a_dxh * axh).sum(0)
        t, a_t = dxh - s1 / n - xhat * s2 / n, a_dxh + a_s1 / n + axh * a_s2 / n
    return {"dalpha": ((dy * q * x).sum(0), ((dy * x).abs() * (1 + p * q * axh)).sum(0)),
            "dx": (dy * gate + rstd * t, dy.abs() * a_gate + rstd * a_t)}


# ---- PReLU --------------------------------------------------------------------------------------------------------------
def prelu64(x, slope, dy=None):
    """x [rows, cols], slope of 1 or cols values.  {"y": one float32 product (equality), "dx": likewise,
    "dslope": (want, A) per column, "dslope_sum": (want, A) over all columns}."""
    xf = x.detach().float().cpu()
    sf = slope.detach().float().cpu().reshape(-1)
    out = {"y": torch.where(xf > 0, xf, sf * xf).double()}
    if dy is not None:
        gf = dy.detach().float().cpu()
        out["dx"] = torch.where(xf > 0, gf, sf * gf).double()
        t = torch.where(xf > 0, torch.zeros_like(xf), gf * xf).double()       # an exact product in float64
        t = torch.where(xf > 0, t, gf.double() * xf.double())
        out["dslope"] = (t.sum(0), t.abs().sum(0))
        out["dslope_sum"] = (t.sum().reshape(1), t.abs().sum().reshape(1))
    return out
