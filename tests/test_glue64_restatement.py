"""oracle/glue64.py against torch float64 autograd on the expressions the reference writes (1e-12 relative): SASRec's
three-statement prologue, ``xi + x0 * h + bias``, the einsum of compressed_interaction_net.py and plain slicing with
autograd's fan-out; then every float32 formula evaluated with torch on the CPU, in the kernel's summation order where an
order exists, against the bounds of that file.  No GPU.

The input builders and shape lists below are the ones tests/test_gpu_glue_forms.py runs the kernels on.

Worst bound_ratio of the float32-on-the-CPU evaluation, per op, over the shapes below and randn / one-signed inputs
(test_float32_formulas_meet_the_bounds recomputes them and fails above 0.5):
  cross forward 0.017     cross dh (row sum, lane walk + butterfly) 0.019     rowscale 0.015      rowscale_seq 0.015
  seq_colsum (32-row partials, then nb partials) 0.027          sum_prefix 0.014
  cin dxk 0.057           cin dx0 0.033 (X_k = X_0: 0.016)
  The one-product outputs (cross dx0 and element-wise dh, rowscale without add at alpha = 1, scale_by_scalar, cin forward,
  single-operand sum_prefix) are bit-equal to ``want.float()``."""
import pytest
import torch

from oracle import glue64 as G
from test_interact64_restatement import one_signed, randn

CROSS_DIMS = [1, 3, 4, 8, 63, 64, 65, 100, 128, 200, 256]
CROSS_ROWS = [1, 5, 257]
ROWSCALE_SHAPES = [(3, 7), (1, 1), (5, 6), (2, 3), (257, 64), (9, 4), (4096, 7)]
SEQ_SHAPES = [(3, 5, 7), (2, 1, 4), (7, 200, 64), (1, 3, 6)]
COLSUM_DIMS = [4, 6, 64]
COLSUM_LENS = [1, 5, 200]
COLSUM_BATCHES = [1, 7, 8, 31, 32, 33, 255, 256, 257, 290]
PREFIX_SHAPES = [(8, 8), (8, 0), (8, 4), (37, 5), (37, 36), (40, 24), (1677, 1664), (1, 1)]
PREFIX_ROWS = [1, 5, 300]
SUBSETS = [(u, v, w) for u in (0, 1) for v in (0, 1) for w in (0, 1)]
CIN_SHAPES = [(1, 1, 1, None), (2, 1, 4, 1), (3, 5, 10, None), (3, 5, 10, 7), (2, 39, 16, 24), (2, 39, 40, 200),
              (2, 39, 64, 256), (2, 130, 8, 130), (2, 130, 8, None)]
SCALAR_NS = [1, 255, 256, 257]


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- input builders (shared with the GPU file) ------------------------------------------------------------------------
def values(shape, seed, kind="randn"):
    return {"randn": randn, "one_signed": one_signed}[kind](shape, seed)


def scales(shape, seed, kind="randn"):
    """General values in [-2, 2] (one-signed: [0.25, 2]) with about one exact zero in five."""
    g = gen(seed)
    s = torch.rand(shape, generator=g) * 4 - 2
    if kind == "one_signed":
        s = s.abs() * 0.875 + 0.25
    s[torch.rand(shape, generator=g) < 0.2] = 0.0
    return s


def cross_case(rows, dim, h_cols, bias=True, seed=0, kind="randn"):
    """(x0, xi, h, bias or None, g)."""
    k = seed * 29 + rows * 3 + dim
    return (values((rows, dim), k, kind), values((rows, dim), k + 1, kind), values((rows, h_cols), k + 2, kind),
            values((dim,), k + 3, kind) if bias else None, values((rows, dim), k + 4, kind))


def rowscale_case(rows, dim, with_add, seed=0, kind="randn"):
    """(x, add or None, s, g)."""
    k = seed * 31 + rows * 5 + dim
    return (values((rows, dim), k, kind), values((rows, dim), k + 1, kind) if with_add else None, scales((rows,), k + 2, kind),
            values((rows, dim), k + 3, kind))


def seq_case(B, L, D, seed=0, kind="randn"):
    """(x [B, L, D], pos [L, D], keep [B, L], g [B, L, D])."""
    k = seed * 37 + B * 7 + L * 3 + D
    return (values((B, L, D), k, kind), values((L, D), k + 1, kind), scales((B, L), k + 2, kind), values((B, L, D), k + 3, kind))


def prefix_case(rows, cols, prefix, seed=0):
    """(base [rows, cols], a [rows, prefix], b [rows, prefix])."""
    k = seed * 41 + rows + cols * 3 + prefix
    return randn((rows, cols), k), randn((rows, prefix), k + 1), randn((rows, prefix), k + 2)


def cin_case(B, F, D, M, seed=0, kind="randn"):
    """(x0 [B, F, D], xk [B D, M] or None, dz [B D, F M])."""
    k = seed * 43 + B + F * 3 + D * 5 + (M or 0)
    return (values((B, F, D), k, kind), None if M is None else values((B * D, M), k + 1, kind),
            values((B * D, F * (M or F)), k + 2, kind))


# ---- against autograd ---------------------------------------------------------------------------------------------------
def close12(got, want, what, A=None):
    """1e-12 relative: to the value, or, where terms cancel, to their absolute sum A."""
    got, want = got.double(), want.double().reshape(got.shape)
    ref = want.abs() if A is None else A.double().reshape(got.shape)
    bad = (got - want).abs() > 1e-12 * ref + 1e-300
    assert not bool(bad.any()), "%s: %d of %d elements" % (what, int(bad.sum()), bad.numel())


def leaf(t):
    return t.float().double().requires_grad_(True)


@pytest.mark.parametrize("B,L,D,alpha", [(3, 5, 7, 7 ** 0.5), (7, 20, 8, 1.0), (33, 4, 6, 8.0)])
def test_sasrec_prologue_vs_autograd(B, L, D, alpha):
    """sasrec.py:68-77: seqs = item_emb(seq) * sqrt(D); seqs += position_emb(positions); seqs *= ~timeline_mask."""
    x, pos, keep, g = seq_case(B, L, D, seed=1)
    al = float(torch.tensor(alpha, dtype=torch.float32))
    e = leaf(x)
    table = leaf(torch.cat([pos, randn((3, D), 5)]))                   # a position table longer than L
    positions = torch.arange(L).unsqueeze(0).repeat(B, 1)
    seqs = e * al
    seqs = seqs + torch.nn.functional.embedding(positions, table)
    seqs = seqs * keep.double().unsqueeze(-1)
    seqs.backward(g.double())
    want, A = G.rowscale_seq(x, pos, keep, alpha)
    close12(want, seqs.detach(), "out", A)
    (de, a_de), (dpos, a_dpos) = G.sasrec_input_bwd(g, keep, alpha)
    close12(de, e.grad, "de", a_de)
    close12(dpos, table.grad[:L], "dpos", a_dpos)
    assert int(table.grad[L:].count_nonzero()) == 0
    w2, a2 = G.rowscale(x, pos.unsqueeze(0).expand(B, L, D), keep, alpha)
    assert torch.equal(w2, want) and torch.equal(a2, A)
    cs, _ = G.seq_colsum(g, keep)
    assert torch.equal(cs, dpos)


@pytest.mark.parametrize("h_cols", [1, None])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("rows,dim", [(5, 1), (5, 3), (7, 64), (3, 100)])
def test_cross_vs_autograd(rows, dim, bias, h_cols):
    x0, xi, h, b, g = cross_case(rows, dim, h_cols or dim, bias, seed=2)
    l0, li, lh = leaf(x0), leaf(xi), leaf(h)
    out = li + l0 * lh
    if b is not None:
        out = out + b.double()
    out.backward(g.double())
    want, A = G.cross_fwd(x0, xi, h, b)
    close12(want, out.detach(), "out", A)
    (dx0, a0), (dh, ah) = G.cross_bwd(x0, h, g)
    close12(dx0, l0.grad, "dx0", a0)
    close12(dh, lh.grad, "dh", ah)
    assert torch.equal(li.grad, g.double())


@pytest.mark.parametrize("B,F,D,M", [(1, 1, 1, None), (2, 1, 4, 1), (3, 5, 10, None), (3, 5, 10, 7), (2, 39, 16, 24)])
def test_cin_vs_the_einsum(B, F, D, M):
    """compressed_interaction_net.py:41-43: einsum("bhd,bmd->bhmd") + view, laid out z[(b, d), h M + m]."""
    x0, xk, dz = cin_case(B, F, D, M, seed=3)
    a = leaf(x0)
    k = None if xk is None else leaf(xk)
    kk = a if k is None else k.view(B, D, -1).transpose(1, 2)                  # [B, M, D]
    z = torch.einsum("bhd,bmd->bhmd", a, kk).reshape(B, -1, D).transpose(1, 2).reshape(B * D, -1)
    z.backward(dz.double())
    want, A = G.cin_fwd(x0, xk)
    close12(want, z.detach(), "z", A)
    (dx0, a0), dk = G.cin_bwd(x0, xk, dz)
    close12(dx0, a.grad, "dx0", a0)
    if k is None:
        assert dk is None
    else:
        close12(dk[0], k.grad, "dxk", dk[1])


@pytest.mark.parametrize("used", SUBSETS)
@pytest.mark.parametrize("rows,cols,n", [(5, 37, 5), (3, 8, 8), (4, 40, 24), (1, 1, 1)])
def test_sum_prefix_vs_plain_slicing(rows, cols, n, used):
    """x, x[:, :n], x[:, :n] with autograd's own fan-out; an unused reader is the absent operand."""
    base, a, b = prefix_case(rows, cols, n, seed=4)
    x = leaf(randn((rows, cols), 9))
    parts = (x, x[:, :n], x[:, :n])
    ws = (base, a, b)
    loss = sum((p * w.double()).sum() for p, w, u in zip(parts, ws, used) if u)
    if any(used):
        loss.backward()
    got = x.grad if x.grad is not None else torch.zeros(rows, cols, dtype=torch.float64)
    want, A = G.sum_prefix(*[w if u else None for w, u in zip(ws, used)], rows=rows, cols=cols, prefix=n)
    close12(want, got, "dx", A)
    if sum(used) <= 1:
        assert torch.equal(want, got)
        assert torch.equal(A, want.abs())


def test_rowscale_and_scalar_vs_torch():
    x, add, s, g = rowscale_case(5, 6, True, seed=5)
    for al in (1.0, 8.0):
        for ad in (add, None):
            want, A = G.rowscale(x, ad, s, al)
            ref = x.double() * al
            if ad is not None:
                ref = ref + ad.double()
            close12(want, ref * s.double().unsqueeze(-1), "rowscale", A)
    sc = torch.tensor(0.37)
    want, A = G.scale_by_scalar(x, sc)
    assert torch.equal(want, x.double() * sc.double()) and torch.equal(A, want.abs())


def test_empty_inputs():
    assert G.seq_colsum(torch.zeros(0, 3, 4), torch.zeros(0, 3))[0].eq(0).all()
    assert G.cin_fwd(torch.zeros(0, 5, 8))[0].shape == (0, 25)
    want, A = G.sum_prefix(None, None, None, 3, 5, 2)
    assert int(want.count_nonzero()) == 0 and int(A.count_nonzero()) == 0


# ---- the float32 formulas, in the kernels' order, against the bounds ------------------------------------------------------
def f32_cross_dh(x0, g):
    """cross_bwd_kernel<64> with h_cols == 1: lane c % 64 adds its products in sequence, then group_sum<64>'s butterfly."""
    rows, dim = x0.shape
    k = -(-dim // 64)
    t = torch.zeros(rows, k * 64)
    t[:, :dim] = g.float() * x0.float()
    t = t.view(rows, k, 64)
    acc = torch.zeros(rows, 64)
    for i in range(k):
        acc = acc + t[:, i]
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lane ^ o]
    return acc[:, :1]


def f32_colsum(g, s):
    """seq_colsum: partials of 32 sequences in ascending order, then the partials in ascending order."""
    B, L, D = g.shape
    t = g.float() * s.float().unsqueeze(-1)
    out = torch.zeros(L, D)
    for b0 in range(0, B, 32):
        p = torch.zeros(L, D)
        for b in range(b0, min(b0 + 32, B)):
            p = p + t[b]
        out = out + p
    return out


def f32_cin_bwd(x0, xk, dz):
    """cin_outer_bwd_kernel: dx0 over m in sequence, dxk over h in sequence; X_k = X_0 adds the two sums."""
    B, F, D = x0.shape
    own = xk is None
    k = x0.float().transpose(1, 2) if own else xk.float().view(B, D, -1)       # [B, D, M]
    M = k.shape[2]
    g = dz.float().view(B, D, F, M)
    x0t = x0.float().permute(0, 2, 1)                                          # [B, D, F]
    d0 = torch.zeros(B, D, F)
    for m in range(M):
        d0 = d0 + g[:, :, :, m] * k[:, :, m:m + 1]
    dk = torch.zeros(B, D, M)
    for h in range(F):
        dk = dk + g[:, :, h, :] * x0t[:, :, h:h + 1]
    if own:
        return (d0 + dk).permute(0, 2, 1), None
    return d0.permute(0, 2, 1), dk.reshape(B * D, M)


def test_float32_formulas_meet_the_bounds():
    worst = {}

    def note(op, got, want, A, C):
        r = G.bound_ratio(got, want, A, C)
        worst[op] = max(worst.get(op, 0.0), r)

    def exact(op, got, want):
        assert torch.equal(got.float(), want.float().reshape(got.shape)), op

    for kind in ("randn", "one_signed"):
        for dim in CROSS_DIMS:
            for rows in CROSS_ROWS:
                for hc in (1, dim):
                    x0, xi, h, b, g = cross_case(rows, dim, hc, True, kind=kind)
                    for bb in (b, None):
                        want, A = G.cross_fwd(x0, xi, h, bb)
                        got = xi + (x0 * h + (bb if bb is not None else torch.zeros(dim)))
                        note("cross forward", got, want, A, G.c_cross_fwd())
                    (dx0, _), (dh, a_dh) = G.cross_bwd(x0, h, g)
                    exact("cross dx0", g * h, dx0)
                    if hc == 1:
                        note("cross dh", f32_cross_dh(x0, g), dh, a_dh, G.c_cross_dh(dim))
                    else:
                        exact("cross dh", g * x0, dh)
        for rows, dim in ROWSCALE_SHAPES:
            for with_add in (True, False):
                for al in (1.0, 8.0):
                    x, add, s, _ = rowscale_case(rows, dim, with_add, kind=kind)
                    want, A = G.rowscale(x, add, s, al)
                    got = al * x
                    if add is not None:
                        got = got + add
                    got = got * s.unsqueeze(-1)
                    if add is None and al == 1.0:
                        exact("rowscale", got, want)
                    note("rowscale", got, want, A, G.c_rowscale())
        for B, L, D in SEQ_SHAPES:
            x, pos, keep, _ = seq_case(B, L, D, kind=kind)
            want, A = G.rowscale_seq(x, pos, keep, 8.0)
            note("rowscale_seq", (8.0 * x + pos.unsqueeze(0)) * keep.unsqueeze(-1), want, A, G.c_rowscale())
        for B in COLSUM_BATCHES:
            for L, D in ((5, 6), (1, 4)):
                _, _, keep, g = seq_case(B, L, D, kind=kind)
                want, A = G.seq_colsum(g, keep)
                note("seq_colsum", f32_colsum(g, keep), want, A, G.c_colsum(B))
        for B, F, D, M in CIN_SHAPES:
            x0, xk, dz = cin_case(B, F, D, M, kind=kind)
            want, _ = G.cin_fwd(x0, xk)
            kk = x0.transpose(1, 2) if xk is None else xk.view(B, D, -1)
            exact("cin forward", (x0.permute(0, 2, 1).unsqueeze(3) * kk.unsqueeze(2)).reshape(want.shape), want)
            (dx0, a0), dk = G.cin_bwd(x0, xk, dz)
            g0, gk = f32_cin_bwd(x0, xk, dz)
            note("cin dx0 own" if xk is None else "cin dx0", g0, dx0, a0, G.c_cin_dx0(F, M or F, xk is None))
            if dk is not None:
                note("cin dxk", gk, dk[0], dk[1], G.c_cin_dxk(F))
    for cols, prefix in PREFIX_SHAPES:
        for rows in (1, 5):
            base, a, b = prefix_case(rows, cols, prefix)
            for used in SUBSETS:
                ops_ = [t if u else None for t, u in zip((base, a, b), used)]
                want, A = G.sum_prefix(*ops_, rows=rows, cols=cols, prefix=prefix)
                got = torch.zeros(rows, cols) if ops_[0] is None else ops_[0].clone()
                for t in ops_[1:]:
                    if t is not None:
                        got[:, :prefix] = got[:, :prefix] + t
                if sum(used) <= 1:
                    exact("sum_prefix", got, want)
                note("sum_prefix", got, want, A, G.c_sum_prefix())
    x = randn((257,), 3)
    exact("scale_by_scalar", x * torch.tensor(0.37), G.scale_by_scalar(x, torch.tensor(0.37))[0])
    print("worst bound_ratio per op: " + "  ".join("%s %.2g" % kv for kv in sorted(worst.items())))
    assert len(worst) == 9
    for op, r in worst.items():
        assert r <= 0.5, "%s: %.3g of its bound on the CPU -- the derivation is wrong" % (op, r)


def test_constants_follow_the_derivations():
    assert G.c_cross_fwd() == G.c_rowscale() == G.c_sum_prefix() == G.C_BOUND == 64
    assert G.c_cross_dh(1) == 64 and G.c_cross_dh(64 * 60) == 68
    assert G.c_colsum(290) == 64 and G.c_colsum(32 * 40) == 74 and G.c_colsum(5) == 64
    assert G.c_cin_dxk(39) == 64 and G.c_cin_dxk(130) == 132
    assert G.c_cin_dx0(39, 256, False) == 258 and G.c_cin_dx0(130, 130, True) == 263 and G.c_cin_dx0(5, 5, True) == 64
