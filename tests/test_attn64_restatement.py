"""oracle/attn64.py against torch float64 autograd (softmax of the masked scores @ v with an injected keep mask, .backward())
at about 1e-12 relative, and its restatement of the attention dispatch (attn_form, attn_chunk) at the boundary values of
the kernels' thresholds.  Runs without a GPU."""
import pytest
import torch

from oracle import attn64 as A64

RTOL = 1e-12


def torch_attention(q, k, v, mask, scale, causal, fill, keep, p_drop, do):
    q, k, v = (t.float().double().requires_grad_() for t in (q, k, v))
    s = A64.f32(scale) * (q @ k.transpose(-1, -2))
    if mask is not None:
        s = s.masked_fill(mask.expand_as(s) == 0, A64.f32(fill))
    if causal:
        s = s.masked_fill(~torch.tril(torch.ones(s.shape[-2:], dtype=torch.bool)), float("-inf"))
    p = torch.softmax(s, -1)
    lse = torch.logsumexp(s, -1)
    if p_drop:
        p = p * keep.double() / (1.0 - A64.p_eff(p_drop))
    o = p @ v
    o.backward(do.float().double())
    return o.detach(), lse.detach(), p.detach(), q.grad, k.grad, v.grad


def rel(got, want, A=None):
    """largest error relative to the largest magnitude (A where given: gradients of peaked rows cancel to far below it)"""
    ref = want.abs().max() if A is None else torch.maximum(A.max(), want.abs().max())
    return float((got - want).abs().max() / ref.clamp_min(1e-300))


CASES = [  # bh, lq, lk, hd, causal, mask kind, fill, p_drop, input kind
    (2, 5, 5, 4, False, None, -1e9, 0.0, "randn"),
    (3, 9, 9, 8, True, None, -1e9, 0.0, "ramp"),
    (2, 7, 12, 16, True, "random", -1e9, 0.0, "randn"),
    (2, 12, 7, 32, True, "rows", -1e9, 0.0, "first"),
    (2, 6, 10, 64, False, "random", float("-inf"), 0.0, "last"),
    (2, 10, 6, 8, False, "rows", -1e9, 0.5, "randn"),
    (3, 33, 33, 32, True, None, -1e9, 0.1, "onehot"),
    (2, 11, 11, 16, True, "random", float("-inf"), 0.5, "randn"),
]


def make_mask(kind, bh, lq, lk, seed, chunk=None):
    """float mask [bh, lq, lk], 0 = masked.  "random": each entry kept with probability 0.7, key 0 always kept (no row is
    hidden entirely, causal or not); "rows": the same, and every third row hides every key; "tile": keys 32 .. 63 (or the
    middle third of a short row) hidden for every row; "chunk0" / "chunklast": every key of the first / last LDS chunk of
    ``chunk`` keys hidden for every row, the rest random (a causal row that ends inside chunk 0 is then hidden entirely)."""
    if kind is None:
        return None
    g = torch.Generator().manual_seed(seed)
    m = (torch.rand(bh, lq, lk, generator=g) < 0.7).float()
    m[:, :, 0] = 1.0
    if kind == "rows":
        m[:, ::3] = 0.0
    if kind in ("chunk0", "chunklast"):
        m[:, :, 0] = (torch.rand(bh, lq, generator=g) < 0.7).float()
        lo = 0 if kind == "chunk0" else (lk - 1) // chunk * chunk
        m[:, :, lo:min(lo + chunk, lk)] = 0.0
    if kind == "tile":
        m = torch.ones(bh, lq, lk)
        lo, hi = (32, 64) if lk > 64 else (lk // 3, max(lk // 3 + 1, 2 * lk // 3))
        m[:, :, lo:hi] = 0.0
    return m


@pytest.mark.parametrize("bh,lq,lk,hd,causal,mkind,fill,p,kind", CASES)
def test_restatement_equals_torch_float64_autograd(bh, lq, lk, hd, causal, mkind, fill, p, kind):
    q, k, v, scale = A64.make_inputs(kind, bh, lq, lk, hd, seed=3)
    mask = make_mask(mkind, bh, lq, lk, 5)
    g = torch.Generator().manual_seed(11)
    keep = (torch.rand(bh, lq, lk, generator=g) >= p) if p else None
    do = torch.randn(bh, lq, hd, generator=g)
    f = A64.attn_fwd(q, k, v, mask, scale, causal, fill, keep, p)
    b = A64.attn_bwd(q, k, v, mask, scale, causal, fill, do, keep, p)
    o, lse, pr, dq, dk, dv = torch_attention(q, k, v, mask, scale, causal, fill, keep, p, do)
    for name, pair, want in (("o", f["o"], o), ("lse", f["lse"], lse), ("p", f["p"], pr), ("dq", b["dq"], dq),
                             ("dk", b["dk"], dk), ("dv", b["dv"], dv)):
        assert bool(torch.isfinite(want).all()), name
        assert rel(pair[0], want, pair[1]) <= RTOL, "%s: %.3e" % (name, rel(pair[0], want, pair[1]))
    for name, (want, A) in list(f.items()) + list(b.items()):
        assert bool((A >= 0).all()) and bool(torch.isfinite(A).all()), name
        if name == "lse":
            continue
        floor = 1.0 / (1.0 - A64.p_eff(p)) if name == "dk" or name == "dq" else 1.0
        assert bool((A * floor * (1 + 1e-12) >= want.abs()).all()), "%s: A is below |want|" % name
    hidden = ~torch.tril(torch.ones(lq, lk, dtype=torch.bool)) if causal else torch.zeros(lq, lk, dtype=torch.bool)
    assert int(torch.count_nonzero(f["p"][1][:, hidden])) == 0 and int(torch.count_nonzero(f["p"][0][:, hidden])) == 0


def test_a_row_hidden_entirely_is_uniform_at_minus_1e9_and_nan_at_minus_inf():
    bh, lq, lk, hd = 2, 6, 5, 8
    q, k, v, scale = A64.make_inputs("randn", bh, lq, lk, hd, seed=1)
    mask = torch.ones(bh, lq, lk)
    mask[:, 2] = 0.0
    do = torch.randn(bh, lq, hd, generator=torch.Generator().manual_seed(2))
    for causal in (False, True):
        f = A64.attn_fwd(q, k, v, mask, scale, causal, -1e9)
        n = min(2, lk - 1) + 1 if causal else lk
        want = torch.zeros(lk, dtype=torch.float64)
        want[:n] = 1.0 / n
        assert torch.allclose(f["p"][0][:, 2], want.expand(bh, lk), rtol=1e-14, atol=0)
        o, lse, pr, dq, dk, dv = torch_attention(q, k, v, mask, scale, causal, -1e9, None, 0.0, do)
        b = A64.attn_bwd(q, k, v, mask, scale, causal, -1e9, do)
        assert rel(b["dq"][0], dq) <= RTOL and rel(b["dk"][0], dk) <= RTOL and rel(b["dv"][0], dv) <= RTOL
        assert int(torch.count_nonzero(dq[:, 2])) == 0          # masked_fill passes nothing back to a replaced score
        f = A64.attn_fwd(q, k, v, mask, scale, causal, float("-inf"))
        o, lse, pr, dq, dk, dv = torch_attention(q, k, v, mask, scale, causal, float("-inf"), None, 0.0, do)
        # torch makes the whole row NaN; the restatement keeps the causally hidden entries of it at exactly zero, so with
        # ``causal`` row 2 is NaN at keys 0 .. 2 only, and dV at the keys that row 2 sees
        vis = torch.ones(lq, lk, dtype=torch.bool).tril() if causal else torch.ones(lq, lk, dtype=torch.bool)
        assert torch.equal(torch.isnan(f["o"][0]), torch.isnan(o)) and bool(torch.isnan(f["o"][0][:, 2]).all())
        want, A = f["p"]
        assert bool(torch.isnan(pr[:, 2]).all()) and int(torch.isnan(pr).sum()) == pr[:, 2].numel()
        assert torch.equal(torch.isnan(want), torch.isnan(pr) & vis) and int(torch.count_nonzero(want[:, ~vis])) == 0
        assert int(torch.count_nonzero(A[:, 2])) == 0
        b = A64.attn_bwd(q, k, v, mask, scale, causal, float("-inf"), do)
        assert not bool(torch.isnan(dq).any()) and bool(torch.isnan(dv).all())
        for name, t in (("dq", dq), ("dk", dk)):
            assert bool(torch.isfinite(b[name][0]).all()) and rel(b[name][0], t) <= RTOL, name
        seen = vis[2].view(1, lk, 1).expand_as(dv)
        assert torch.equal(torch.isnan(b["dv"][0]), seen)
        if causal:      # the keys row 2 does not see: what torch gives without that row's cotangent
            do0 = do.clone()
            do0[:, 2] = 0.0
            m1 = mask.clone()
            m1[:, 2] = 1.0
            dv0 = torch_attention(q, k, v, m1, scale, causal, float("-inf"), None, 0.0, do0)[5]
            assert rel(b["dv"][0][~seen], dv0[~seen]) <= RTOL


def test_attn_chunk_and_the_dispatch_at_their_boundaries():
    assert [A64.attn_chunk(10 ** 6, hd) for hd in (4, 8, 16, 32, 64)] == [2456, 1360, 720, 368, 184]
    assert A64.attn_chunk(9, 8) == 16 and A64.attn_chunk(184, 64) == 184 and A64.attn_chunk(185, 64) == 184
    F = A64.attn_form
    for hd, C in ((4, 2456), (8, 1360), (16, 720), (32, 368), (64, 184)):
        assert F(1, C, C, hd, False, hd >= 32, False) == ("valu:1", "valu:1,1")
        assert F(1, C + 1, C + 1, hd, True, hd >= 32, False) == ("valu:2", "valu:2,2")
        assert F(1, 5, C + 9, hd, False, True, False) == ("valu:2", "valu:2,1")
    assert F(2, 400, 400, 64, False, False, False) == ("valu:3", "valu:3,3")
    assert F(2, 513, 513, 16, False, False, False).fwd == "valu:1"            # (720 rows a chunk: still one)
    # what keeps a matrix-core shape on the VALU kernels: a mask, probabilities, no lse buffer, lq != lk, L > 256, hd < 32
    assert F(5, 200, 200, 64, True, False, False) == ("planes", "mfma:split")
    assert F(5, 200, 200, 64, True, True, False) == ("valu:2", "valu:2,2")
    assert F(5, 200, 200, 64, True, False, True) == ("valu:2", "mfma:split")
    assert F(5, 200, 200, 64, True, False, False, has_lse=False).fwd == "valu:2"
    assert F(5, 200, 199, 64, True, False, False).fwd == "valu:2" and F(5, 257, 257, 32, True, False, False).fwd == "valu:1"
    assert F(5, 64, 64, 16, True, False, False) == ("valu:1", "valu:1,1")
    # hd 32: resident, the causal forward splits from three tiles on
    for L, causal, want in ((1, True, "resident"), (64, True, "resident"), (65, True, "resident:split2"),
                            (256, True, "resident:split2"), (65, False, "resident"), (256, False, "resident")):
        assert F(5, L, L, 32, causal, False, False).fwd == want and F(300, L, L, 32, causal, False, False).fwd == want
    assert F(5, 64, 64, 32, True, False, False).bwd == "mfma" and F(5, 65, 65, 32, True, False, False).bwd == "mfma:split"
    assert F(5, 200, 200, 32, False, False, False).bwd == "mfma"
    # hd 64 causal: resident to 64, the ring per nT to 192, planes to 224, resident (unsplit) beyond
    want = {1: "resident", 64: "resident", 65: "stream:3", 96: "stream:3", 97: "stream:4", 128: "stream:4", 129: "stream:5",
            160: "stream:5", 161: "stream:6", 192: "stream:6", 193: "planes", 224: "planes", 225: "resident", 256: "resident"}
    for L, w in want.items():
        assert F(5, L, L, 64, True, False, False).fwd == w, L
    assert F(515, 200, 200, 64, True, False, False).fwd == "planes:loop" and F(512, 200, 200, 64, True, False, False).fwd == "planes"
    assert F(513, 200, 200, 64, True, False, False).fwd == "planes:loop"
    # the looping forward: more than 256 sequences and Lp >= 160
    for L, w in ((128, "resident"), (129, "loop:8"), (160, "loop:8"), (161, "loop:6"), (192, "loop:6"), (193, "loop:7"),
                 (224, "loop:7"), (225, "loop:8"), (256, "loop:8")):
        assert F(257, L, L, 64, False, False, False).fwd == w, L
        assert F(256, L, L, 64, False, False, False).fwd == "resident"
    assert F(257, 225, 225, 64, True, False, False).fwd == "loop:8" and F(300, 256, 256, 64, True, False, False).fwd == "loop:8"
    assert F(257, 200, 200, 64, True, False, False).fwd == "planes"
    # split = 1 (looping and split) is never formed: attn_form asserts it on the way
    for L in range(1, 257):
        for bh in (5, 257, 600):
            for hd in (32, 64):
                for causal in (False, True):
                    F(bh, L, L, hd, causal, False, False)
    # constants: the floor, and the chains where they pass it
    assert A64.c_fwd(F(5, 64, 64, 32, False, False, False), 64, 32) == 64
    assert A64.c_fwd(F(5, 256, 256, 64, False, False, False), 256, 64) == 32 + 2 + 80
    assert A64.c_fwd(F(5, 256, 256, 32, True, False, False), 256, 32) == 16 + 2 + 90
    assert A64.c_fwd(F(5, 200, 200, 64, True, False, False), 200, 64) == 32 + 2 + 70 + 1
    assert A64.c_fwd(F(1, 2457, 2457, 4, True, False, False), 2457, 4) == 2 + 2 + 5 * 308
    assert abs(A64.p_eff(0.1) - 6554 / 65536) < 1e-15 and A64.p_eff(0.5) == 0.5
