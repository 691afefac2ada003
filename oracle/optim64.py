"""Float64 restatement of the sparse-row optimiser step (rbx_optim.hip: opt_apply behind rbx_embed_sparse_update,
rbx_embed_csr_sparse_update and rbx_fm_sparse_update) and of the step size rbx_opt_advance writes, in the conventions of
oracle/score64.py:

    |got - want| <= C * eps32 * A + tiny          A: the sum of the absolute values of the terms that were added

Plain torch float64 on the CPU; every input -- tables, state, gradients AND the scalars lr, beta1, beta2, eps,
weight_decay, lr_decay, which the C ABI carries as floats -- is rounded to float32 first; no product code is imported.
Every function returns ``(want, A)`` pairs.

The contract
    ``rows`` are the rows the batch LOOKED UP (in range, neither padding_idx nor a masked id).  Each of them is stepped
    exactly once however often it is named, and whatever its summed gradient is: a looked-up row whose gradient is exactly
    zero still decays Adam's moments and moves by lr m' / (sqrt(v') + eps) -- torch.optim.SparseAdam on a coalesced sparse
    gradient does the same.  (recbox_amd.optim's dense fallback selects rows by g != 0 and leaves such a row alone: see
    that module's docstring.)  Every other row of the table and of the state is returned untouched (A = 0: bit-identical).
    weight_decay applies to all three rules: g' = g + wd w.

Definitions, per element of a stepped row
    g' = g + wd w                                          A_g = |g| + |wd w|
    SGD      w' = w - lr g'                                A_w = |w| + lr A_g
    Adagrad  s' = s + g'^2                                 A_s = s + g'^2 + 2 |g'| A_g
             u  = g' / (sqrt(s') + eps)
             w' = w - lr u                                 A_w = |w| + lr (A_g / (sqrt(s') + eps) + |u| (1 + A_s / (2 s')))
    Adam     m' = b1 m + (1 - b1) g'                       A_m = b1 |m| + (1 - b1) A_g
             v' = b2 v + (1 - b2) g'^2                     A_v = b2 v + (1 - b2) (g'^2 + 2 |g'| A_g)
             u  = m' / (sqrt(v') + eps)
             w' = w - lr u                                 A_w = |w| + lr (A_m / (sqrt(v') + eps) + |u| (1 + A_v / (2 v')))
    g'^2 is a product of one rounded number with itself: a rounding of g' of size eps32 A_g moves it by 2 |g'| eps32 A_g,
    the only place where a cancellation (g against wd w) feeds a sum of non-negative terms; hence the third term of A_s
    and A_v.  In A_w the first term in the bracket carries the error of the numerator, |u| the roundings of sqrt, + eps,
    the division and the product with lr, and |u| A / (2 s') what the error of s' (v') does through the square root (0
    where s' = 0: then A is 0 too).  1 - b1 and 1 - b2 are exact in float32 for betas in [0.5, 1) and for 0.

Constant
    Every element is computed by one thread from its own inputs: at most 2 roundings for g', 3 for m', 4 for v' (s': 2),
    then sqrt, + eps, lr *, /, - : 13 in the longest chain (Adam's w), each already weighted by the A it acts on.
    C = C_BOUND = 64, the project's floor, for every form (scalar / float4 lanes, the dim-1 LR column, tier A and tier B:
    the lane group only decides WHICH thread holds an element).
    sqrtf and / : recbox_amd/build.py compiles with -O3 and nothing else that touches floating point; hipcc's default is
    -fhip-fp32-correctly-rounded-divide-sqrt, so both are correctly rounded on the device and no allowance T is added.
    (Contraction of a * b + c into an fma is on by default and only removes roundings.)

The step size of step t (rbx_opt_advance; by value: recbox_amd.optim._step_size)
    SGD      lr
    Adagrad  lr / (1 + (t - 1) lr_decay)
    Adam     lr sqrt(1 - b2^t) / (1 - b1^t)
    as float64 functions of the float32 lr, betas and lr_decay.  Bound: RELATIVE error <= eps32 * K with
        Adam     K = (1 + P b2^t / (1 - b2^t)) / 2 + (1 + P b1^t / (1 - b1^t)) + 4
        Adagrad  K = 4,  SGD  K = 0 (the value is copied)
    from the conditioning of 1 - b^t: a result of powf that is off by P eps32 b^t moves 1 - b^t by that much, the
    subtraction rounds once; the square root halves a relative error; + 4 for sqrt, the division, the product with lr
    and the final store -- there is no floor of 64 here, the chain is six operations long.  (b = 0: powf(0, t) = 0 and the
    factor is exactly 1.)  P = 1 + T_POW: one ulp for the rounding of the result plus the allowance for the library's
    powf, whose accuracy cannot be derived from this repository.  T_POW is MEASURED: float32 pow on the CPU against
    float64 pow of the same float32 arguments, over the bases 0.5, 0.9, 0.999, 0.9999 and t = 1 .. 40, 4990 .. 5010:
    worst 0.50 ulp (it is correctly rounded here); T_POW = 2 >= 4 x 0.50
    (tests/test_optim64_restatement.py::test_float32_pow_and_the_allowance recomputes it and fails if 4 x the figure
    exceeds T_POW; the 4 x is there because the device library may differ from the host's by a few ulp).

Verdicts (tests/test_gpu_optim_forms.py, MI355X)
    (a) opt_advance_kernel's float32 step size stays inside this bound at every tested t (1 .. 40 and 5001 .. 5003, Adam
        (0.9, 0.999), (0.5, 0.9999), b1 = 0; Adagrad lr_decay 0 and 0.1; SGD): the kernel is kept as it is.  The by-value
        (worst err / K: 0.20).  The by-value optimiser computed its step size in double from DOUBLE betas: 0.999 and
        float32(0.999) differ by 1.3e-8, which moves 1 - b2^t by t b2^(t - 1) 1.3e-8 -- 53 to 56 eps32 of the step size (6.4e-6
        relative) at every t up to a few hundred, while K falls from 1531 at t = 1 to 53 at t = 31, 42 at t = 40 and 6.4 at
        t = 1000.  From step 31 on that is outside the bound (tests/test_optim64_restatement.py recomputes it), so
        recbox_amd.optim now rounds lr, the betas and lr_decay to float32 before _step_size, and its dense fallback takes
        1 - beta from the rounded betas as the kernels do: the same numbers the kernels get through the ABI, one trajectory
        whether the step is captured or not.
    (b) The record paths (sorted pairs, tier-A bitmaps) step every looked-up row, zero gradient or not: that is the
        contract above and what the tests pin.  The dense fallback (and its union path, which cannot tell a padding id
        from a looked-up row with a zero gradient without the lookups' descriptors) selects rows by g != 0 and leaves
        such a row alone; recbox_amd/optim.py's docstring says so.

Multi-step tests apply this file one step at a time to the device's own previous table and state: bounds do not compound.
"""
import torch

from oracle.fm64 import C_BOUND, EPS32, TINY  # noqa: F401  (one set of conventions)

SGD, ADAGRAD, ADAM = 0, 1, 2
T_POW = 2


def _r(x):
    """float32-rounded, then float64, on the CPU."""
    return x.detach().float().double().cpu()


def _s(v):
    return float(torch.tensor(float(v), dtype=torch.float32))


def step_rows(kind, w, g, rows, s1=None, s2=None, lr=0.0, beta1=0.0, beta2=0.0, eps=0.0, weight_decay=0.0):
    """One step of rule ``kind`` on ``rows`` (any integer tensor / list; duplicates count once) of the table ``w`` [V, D]
    (or [V]) with the dense gradient ``g`` and the state ``s1`` (Adagrad's sum, Adam's m) / ``s2`` (Adam's v).
    Returns ((w', A_w), (s1', A_s1), (s2', A_s2)); state the rule does not have comes back as (None, None)."""
    lr, b1, b2, eps, wd = _s(lr), _s(beta1), _s(beta2), _s(eps), _s(weight_decay)
    w0, g0 = _r(w), _r(g)
    rows = torch.unique(torch.as_tensor(rows).detach().cpu().long().reshape(-1))
    assert rows.numel() == 0 or (int(rows.min()) >= 0 and int(rows.max()) < w0.shape[0])
    wr, gr = w0[rows], g0[rows]
    gp = gr + wd * wr
    a_g = gr.abs() + (wd * wr).abs()
    out_w, a_w = w0.clone(), torch.zeros_like(w0)
    st = [(None, None), (None, None)]

    def through_sqrt(a, x):          # A / (2 x), 0 where x == 0 (then A == 0)
        return torch.where(x > 0, a / (2 * x.clamp_min(1e-300)), torch.zeros_like(x))

    if kind == SGD:
        out_w[rows] = wr - lr * gp
        a_w[rows] = wr.abs() + lr * a_g
    elif kind == ADAGRAD:
        s0 = _r(s1)
        sr = s0[rows]
        sn = sr + gp * gp
        a_s = sr + gp * gp + 2 * gp.abs() * a_g
        den = sn.sqrt() + eps
        u = gp / den
        out_w[rows] = wr - lr * u
        a_w[rows] = wr.abs() + lr * (a_g / den + u.abs() * (1 + through_sqrt(a_s, sn)))
        o1, a1 = s0.clone(), torch.zeros_like(s0)
        o1[rows], a1[rows] = sn, a_s
        st[0] = (o1, a1)
    elif kind == ADAM:
        m0, v0 = _r(s1), _r(s2)
        mr, vr = m0[rows], v0[rows]
        mn = b1 * mr + (1 - b1) * gp
        a_m = b1 * mr.abs() + (1 - b1) * a_g
        vn = b2 * vr + (1 - b2) * gp * gp
        a_v = b2 * vr.abs() + (1 - b2) * (gp * gp + 2 * gp.abs() * a_g)
        den = vn.sqrt() + eps
        u = mn / den
        out_w[rows] = wr - lr * u
        a_w[rows] = wr.abs() + lr * (a_m / den + u.abs() * (1 + through_sqrt(a_v, vn)))
        o1, a1, o2, a2 = m0.clone(), torch.zeros_like(m0), v0.clone(), torch.zeros_like(v0)
        o1[rows], a1[rows], o2[rows], a2[rows] = mn, a_m, vn, a_v
        st = [(o1, a1), (o2, a2)]
    else:
        raise ValueError("unknown rule %r" % (kind,))
    return (out_w, a_w), st[0], st[1]


def step_size(kind, lr, beta1=0.0, beta2=0.0, lr_decay=0.0, t=1):
    """(the step size of step t, K): |got - want| <= K * eps32 * |want|."""
    lr, b1, b2, dec = _s(lr), _s(beta1), _s(beta2), _s(lr_decay)
    t = int(t)
    if kind == SGD:
        return lr, 0.0
    if kind == ADAGRAD:
        return lr / (1.0 + (t - 1) * dec), 4.0
    if kind != ADAM:
        raise ValueError("unknown rule %r" % (kind,))
    p = 1.0 + T_POW

    def cond(b):
        bt = b ** t
        return 1.0 + p * bt / (1.0 - bt)

    return lr * (1.0 - b2 ** t) ** 0.5 / (1.0 - b1 ** t), cond(b2) / 2 + cond(b1) + 4.0


def bound(A, C=C_BOUND):
    return C * EPS32 * A + TINY
