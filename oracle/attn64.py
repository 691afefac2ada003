"""Float64 restatement of the fused softmax attention (rbx_attn.hip, rbx_attn_mfma.hip, rbx_attn_stream.h,
rbx_attn_planes.h) and of its gradients for a given cotangent dO, with a bound per element in the conventions of
oracle/fm64.py, oracle/interact64.py and oracle/norm64.py:

    |got - want| <= C * eps32 * A + tiny

``A == 0`` means exactly zero.  Inputs are rounded to float32 first, no product code is imported, there is no autograd and
everything is float64 on the CPU; every function returns ``(want, A)`` pairs.

Operation.  s_ij = scale <q_i, k_j>; an entry whose mask is 0 gets s_ij = mask_fill (as float32); with ``causal`` key j > i
is hidden (torch.tril(ones(lq, lk)), also where lq != lk); p = softmax over the visible keys, lse = log sum exp.  Dropout
multiplies p by keep / (1 - p_eff), p_eff = round(p_drop * 65536) / 65536 (the 16-bit threshold of make_drop); the
normaliser is the undropped sum and the probabilities returned are the dropped ones.  o = pd v.  Backward, by hand:
    dV = pd^T dO          dP = (dO v^T) keep / (1 - p_eff)          D_i = sum_d dO_id o_id  (= rowsum(p dP))
    dS = p (dP - D), and zero where the mask put mask_fill (masked_fill passes no gradient to the score it replaced;
    with a row that is only partly masked p is zero there anyway, a row that is masked entirely is where it matters)
    dQ = scale dS k       dK = scale dS^T q
A row that mask_fill = -inf hides entirely is NaN in o and in p at its causally visible keys, and -inf in lse, as torch's
softmax and logsumexp of a row of -inf are; a causally hidden entry is exactly zero in EVERY row (torch's softmax makes
those NaN too in such a row; the kernels never touch them, and the row's o is NaN either way).  dV, which sums p over the
rows, is therefore NaN at every key such a row sees; dS is zero there like at every masked entry, so dQ and dK stay
finite.  ``want`` holds the NaN / -inf and A is zero.

Magnitudes.  A_s = scale sum_d |q||k| (zero where the score is mask_fill itself: that value is not computed).
A probability is exp(s - lse): an error ds of its score and dlse = sum_j p_j ds_j of the row move it by p (ds - dlse), so its
relative error carries A_s of its own score plus the p-weighted mean of A_s over the row, Abar.  Two more terms come from
how the kernels evaluate it: __expf(x) is exp2 of the ROUNDED product x log2(e), a relative error of |x| u, and the online
softmax's chain exp(s - m_1) exp(m_1 - m_2) ... has arguments of one sign that add up to s - m, so the chain costs
|s - m| u <= (|s - lse| + log n) u whatever its length; and the roundings of exp itself, of the normaliser and of the
rescales are relative to p: the 1.  So
    r_ij  = 1 + A_s,ij + Abar_i + |s_ij - lse_i|           A_p = p r (times keep / (1 - p_eff))
    A_lse = 1 + |lse| + Abar        (m + log l: the rounding of the sum at |lse|, l's relative error, the scores' errors)
    A_o   = sum_j A_p,ij |v_j|
    A_dV  = sum_i A_p,ij |dO_i|
    A_dP  = keep / (1 - p_eff) sum_d |dO||v|     A_D = sum_d |dO| A_o   (the kernels form D from THEIR o)
    A_dS  = p (r |dP - D| + A_dP + A_D)   (p's relative error on the difference as it is, the roundings of dP and of D on
            their own magnitudes; zero where dS is)       A_dQ = scale sum_j A_dS |k_j|      A_dK = scale sum_i A_dS |q_i|
Causal-hidden and -inf-masked entries have A = 0: the returned probabilities there must be exactly zero.

Constants, read from the kernels (never fitted to what they return), in units of eps32 = 2 u, floor C_BOUND = 64:
    a score            hd products and additions in an unknown order, q scale rounded first: (hd + 2) u = hd / 2 + 1
    VALU forward       (rbx_attn.hip) one lane owns a row and adds key after key: an 8-key step is 8 dependent additions
                       into o and l, one rescale and the exps' own rounding, 5 eps32 a step, and the steps of all chunks
                       follow each other (a chunk boundary is one more rescale, inside the step's 5):
                       c_fwd = max(64, hd / 2 + 2 + 5 ceil(lk / 8))
    matrix cores       a 32-key tile is 16 dependent MFMA steps (8 eps32), a rescale and the exps (2): 10 a tile; the tiles
                       of a row follow each other, the split forms add one merge of two partial (m, l, O) triples (one more
                       rescale and addition, counted as a tile): c_fwd = max(64, hd / 2 + 2 + 10 (nT + merge)), nT = ceil(L / 32)
    bf16 planes        (rbx_attn_planes.h, and every tile product RBX_ATTN_BF16X6 names) x = h + m + l with bf16 h = rn(x),
                       m = rn(x - h), l = rn(x - h - m): |m| <= 2^-9 |x|, |l| <= 2^-18 |x|, |x - h - m - l| <= 2^-27 |x|.  Six of
                       the nine cross products are kept; dropped are m l', l m', l l' and the two residuals: at most
                       (2 2^-27 + 2^-36 + 2 2^-27) |x y| < 2^-25 |x y| = eps32 / 4 a product, against eps32 / 2 for the f32
                       rounding it replaces.  K Q^T and V^T P^T each take it once: + 1 covers both.  c_planes = c_mfma + 1.
    backward           dS needs s (hd / 2 + 1), dP (hd / 2 + 1) and D, whose o carries the forward's constant; the sums over
                       keys (dQ) and queries (dK, dV) are sequential on the VALU route (max(lq, lk) / 2) and 10 a tile plus
                       one merge on the matrix cores, whose products are bf16 planes (+ 1):
                       c_bwd = c_fwd + hd + 4 + (max(lq, lk) / 2  |  10 (nT + 1) + 1)

Dispatch (``attn_form`` restates rbx_attn_dropout_fwd / _bwd and run_fwd / run_bwd; the tests assert it per case):
    matrix cores iff no mask, no probabilities asked for, an lse buffer, lq == lk <= 256, hd in {32, 64}; else VALU with
    chunks of attn_chunk(rows, hd) rows (2456, 1360, 720, 368, 184 at hd 4 .. 64): the forward and dQ chunk the keys, dK|dV
    the queries.  hd 64 causal: nT = 7 -> planes (a workgroup per PAIR of sequences, min(pairs, 256) workgroups: it loops
    from 513 sequences on), nT 3 .. 6 -> streamed ring ((nT + 1) 64 threads, a pair per workgroup).  Otherwise resident:
    hd 64 with more than 80 KB of K, V rows (Lp >= 160) and more than 256 sequences loops with a prefetch of
    NPF = Lp / 32 float4 per thread (instantiated for 6, 7, 8; Lp = 160 has npf = 5 and runs the NPF = 8 body: its three
    extra loads per thread are clamped to row L - 1 by prefetch_rows and never committed, commit_rows writes i < Lp 16 only
    -- wasteful, not wrong), else one workgroup per sequence.  Causal L > 64 splits the heavy tiles over both wavefronts of
    a SIMD: the forward merges through the K rows (split = 2) where the four slots fit 160 KB beside K and V (always at hd 32,
    never at hd 64 nT = 8), the backward kernels always.  split = 1 (looping AND split) is unreachable: hd 32 never loops,
    hd 64 causal nT 3 .. 7 goes to the ring kernels, nT = 8 does not fit the slots, nT <= 2 does not split.
"""
import math
from collections import namedtuple

import torch

from oracle.fm64 import C_BOUND, EPS32, TINY, bound_ratio  # noqa: F401
from oracle.interact64 import ratios  # noqa: F401

K_CUS = 256
K_TILE = 32
KEY_BLOCK = 8


def _r(x):
    return x.detach().float().double().cpu()


def f32(v):
    return float(torch.tensor(float(v), dtype=torch.float32))


def p_eff(p_drop):
    thr = min(int(f32(f32(p_drop) * 65536.0) + 0.5), 65535)
    return thr / 65536.0


# ---- dispatch ------------------------------------------------------------------------------------------------------------
def attn_chunk(rows, hd):
    c = (96 * 1024) // (4 * (2 * hd + 2)) // KEY_BLOCK * KEY_BLOCK
    need = -(-rows // KEY_BLOCK) * KEY_BLOCK
    return min(c, need)


Form = namedtuple("Form", "fwd bwd")


def attn_form(bh, lq, lk, hd, causal, has_mask, want_probs, has_lse=True):
    """Form(fwd, bwd): fwd one of "valu:<key chunks>", "resident", "resident:split2", "loop:<NPF>", "stream:<nT>", "planes",
    "planes:loop"; bwd "valu:<key chunks>,<query chunks>", "mfma" or "mfma:split"."""
    assert hd in (4, 8, 16, 32, 64)
    mfma = (not has_mask) and (not want_probs) and lq == lk and lq <= 256 and hd in (32, 64)
    nk = -(-lk // attn_chunk(lk, hd))
    nq = -(-lq // attn_chunk(lq, hd))
    bwd = "valu:%d,%d" % (nk, nq)
    if (not has_mask) and lq == lk and lq <= 256 and hd in (32, 64):
        bwd = "mfma:split" if (causal and lq > 2 * K_TILE) else "mfma"
    if not (mfma and has_lse):
        return Form("valu:%d" % nk, bwd)
    L = lq
    nT = -(-L // K_TILE)
    Lp = nT * K_TILE
    if hd == 64 and causal:
        if nT == 7:
            return Form("planes:loop" if (bh + 1) // 2 > K_CUS else "planes", bwd)
        if 3 <= nT <= 7:
            return Form("stream:%d" % nT, bwd)
    lds = 2 * Lp * (hd + 1) * 4
    lds_split = lds + 4 * (hd * 32 + 128) * 4
    split_on = bool(causal) and L > 2 * K_TILE and lds_split <= 160 * 1024
    if hd == 64 and lds > 80 * 1024 and bh > K_CUS:
        npf = Lp * (hd // 4) // 512
        assert not split_on, "split = 1: believed unreachable"
        return Form("loop:%d" % (npf if npf in (6, 7) else 8), bwd)
    return Form("resident:split2" if split_on else "resident", bwd)


def c_fwd(form, lk, hd):
    kind = form.fwd.split(":")[0]
    if kind == "valu":
        return max(C_BOUND, hd // 2 + 2 + 5 * (-(-lk // KEY_BLOCK)))
    nT = -(-lk // K_TILE)
    c = hd // 2 + 2 + 10 * (nT + (1 if form.fwd == "resident:split2" else 0))
    return max(C_BOUND, c + (1 if kind == "planes" else 0))


def c_bwd(form, lq, lk, hd):
    if form.bwd.startswith("valu"):
        return c_fwd(form, lk, hd) + hd + 4 + max(lq, lk) // 2
    return c_fwd(form, lk, hd) + hd + 4 + 10 * (-(-lk // K_TILE) + 1) + 1


# ---- the operation -------------------------------------------------------------------------------------------------------
def _scores(q, k, mask, scale, causal, mask_fill):
    q, k = _r(q), _r(k)
    lq, lk = q.shape[-2], k.shape[-2]
    sc = f32(scale)
    s = sc * (q @ k.transpose(-1, -2))
    a_s = abs(sc) * (q.abs() @ k.abs().transpose(-1, -2))
    filled = torch.zeros_like(s, dtype=torch.bool)
    if mask is not None:
        filled = (_r(mask) == 0).expand_as(s).clone()
        s = torch.where(filled, torch.full_like(s, f32(mask_fill)), s)
        a_s = torch.where(filled, torch.zeros_like(a_s), a_s)
    hidden = torch.zeros_like(filled)
    if causal:
        hidden = ~torch.tril(torch.ones(lq, lk, dtype=torch.bool)).expand_as(s)
        s = s.masked_fill(hidden, float("-inf"))
    return q, k, s, a_s, filled, hidden


def _softmax(s, a_s, hidden):
    """p, lse, r (the relative-error weight of p), abar; rows with no finite score are NaN."""
    m = s.max(-1, keepdim=True).values
    dead = torch.isinf(m) & (m < 0)
    e = torch.exp(s - torch.where(dead, torch.zeros_like(m), m))
    l = e.sum(-1, keepdim=True)
    p = e / l
    lse = m + torch.log(l)
    abar = (p * a_s).sum(-1, keepdim=True)
    gap = torch.where(p > 0, (s - lse).abs(), torch.zeros_like(s))
    gap = torch.where(torch.isfinite(gap), gap, torch.zeros_like(gap))
    r = 1.0 + a_s + abar + gap
    nan = torch.full_like(p, float("nan"))
    p = torch.where(dead & ~hidden, nan, p)      # (a causally hidden entry is exactly zero, also in such a row)
    p = torch.where(hidden, torch.zeros_like(p), p)
    lse = torch.where(dead, torch.full_like(lse, float("-inf")), lse)          # (torch.logsumexp of a row of -inf)
    return p, lse, r, abar, dead


def _keep_scale(keep, p_drop, like):
    if keep is None or not p_drop:
        return torch.ones_like(like)
    return keep.detach().double().cpu().expand_as(like) / (1.0 - p_eff(p_drop))


def attn_fwd(q, k, v, mask, scale, causal, mask_fill, keep=None, p_drop=0):
    """{"o", "lse", "p"} -> (want, A).  q [..., lq, hd], k, v [..., lk, hd], mask broadcastable to [..., lq, lk] (0 = masked)
    or None; keep: the kernel's dropout mask (bool [..., lq, lk]) when p_drop > 0."""
    v = _r(v)
    q, k, s, a_s, filled, hidden = _scores(q, k, mask, scale, causal, mask_fill)
    p, lse, r, abar, dead = _softmax(s, a_s, hidden)
    ks = _keep_scale(keep, p_drop, p)
    pd = p * ks
    a_p = torch.where(dead, torch.zeros_like(p), p.nan_to_num(0.0) * r * ks)
    o = pd @ v
    a_o = a_p @ v.abs()
    a_lse = torch.where(dead, torch.zeros_like(lse), 1.0 + lse.nan_to_num(0.0).abs() + abar.nan_to_num(0.0))
    return {"o": (o, a_o), "lse": (lse.squeeze(-1), a_lse.squeeze(-1)), "p": (pd, a_p)}


def attn_bwd(q, k, v, mask, scale, causal, mask_fill, do, keep=None, p_drop=0):
    """{"dq", "dk", "dv"} -> (want, A) for the cotangent ``do`` of o."""
    v, do = _r(v), _r(do)
    q, k, s, a_s, filled, hidden = _scores(q, k, mask, scale, causal, mask_fill)
    p, lse, r, abar, dead = _softmax(s, a_s, hidden)
    sc = f32(scale)
    ks = _keep_scale(keep, p_drop, p)
    pd = p * ks
    p0 = torch.where(dead, torch.zeros_like(p), p.nan_to_num(0.0))
    a_p = p0 * r * ks
    o = pd @ v
    a_o = a_p @ v.abs()
    dv = pd.transpose(-1, -2) @ do
    a_dv = a_p.transpose(-1, -2) @ do.abs()
    dp = (do @ v.transpose(-1, -2)) * ks
    a_dp = (do.abs() @ v.abs().transpose(-1, -2)) * ks
    D = (do * o).sum(-1, keepdim=True)
    a_D = (do.abs() * a_o).sum(-1, keepdim=True)
    ds = p * (dp - D)
    ds = torch.where(filled, torch.zeros_like(ds), ds)          # (also in a NaN row: masked_fill's backward writes zeros)
    gapd = torch.where(p0 > 0, (dp - D).abs(), torch.zeros_like(p0)).nan_to_num(0.0)
    a_ds = torch.where(filled, torch.zeros_like(p0), p0 * (r * gapd + a_dp + a_D))
    dq = sc * (ds @ k)
    a_dq = abs(sc) * (a_ds @ k.abs())
    dk = sc * (ds.transpose(-1, -2) @ q)
    a_dk = abs(sc) * (a_ds.transpose(-1, -2) @ q.abs())
    return {"dq": (dq, a_dq), "dk": (dk, a_dk), "dv": (dv, a_dv)}


# ---- inputs of the tests (shared by the CPU and the GPU file) ------------------------------------------------------------
KINDS = ("randn", "first", "last", "ramp", "onehot", "first200", "last200")


def make_inputs(kind, bh, lq, lk, hd, seed, peak=60.0):
    """(q, k, v, scale) float32 on the CPU.  "randn": scores O(1).  "first" / "last" / "ramp": q = a u + noise, k = b u + noise
    along one unit direction u, so s_ij ~ peak sign(a_i) b_j: b is 1 at the first / last key (|b| <= 0.5 elsewhere), or rises
    to 1 along the keys -- for a causal row the maximum is then on the diagonal and the running maximum moves at every step;
    rows with a_i < 0 have their maximum elsewhere, at -peak b_j.  "onehot": q_i = g k_pi(i) with unit keys, p ~ 1 on one
    visible key.  "first200" / "last200": the same with peak = 200, so that the first (last) keys of a row lead the others by
    more than 88 = log(FLT_MAX): a merge of partial (m, l, O) triples that rescales to the smaller maximum overflows."""
    if kind.endswith("200"):
        kind, peak = kind[:-3], 200.0
    g = torch.Generator().manual_seed(1000 * seed + 7 * lq + lk + hd)
    scale = hd ** -0.5
    v = torch.randn(bh, lk, hd, generator=g)
    if kind == "randn":
        return torch.randn(bh, lq, hd, generator=g), torch.randn(bh, lk, hd, generator=g), v, scale
    if kind == "onehot":
        k = torch.randn(bh, lk, hd, generator=g)
        k = k / k.norm(dim=-1, keepdim=True)
        i = torch.arange(lq)
        pi = (i * 7 + 3) % (torch.minimum(i, torch.full_like(i, lk - 1)) + 1)
        amp = math.sqrt(40.0 / scale)
        return amp * k[:, pi], amp * k, v, scale
    u = torch.randn(hd, generator=g)
    u = u / u.norm()
    amp = math.sqrt(peak / scale)
    a = (torch.rand(bh, lq, 1, generator=g) * 0.5 + 0.5) * torch.where(torch.rand(bh, lq, 1, generator=g) < 0.75, 1.0, -1.0)
    if kind == "ramp":
        b = ((torch.arange(lk).float() + 1) / lk).view(1, lk, 1).expand(bh, lk, 1).clone()
    else:
        b = torch.rand(bh, lk, 1, generator=g) - 0.5
        b[:, 0 if kind == "first" else lk - 1] = 1.0
    q = amp * a * u + 0.1 * torch.randn(bh, lq, hd, generator=g)
    k = amp * b * u + 0.1 * torch.randn(bh, lk, hd, generator=g)
    return q, k, v, scale
