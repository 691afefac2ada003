"""The fused attention (rbx_attn.hip, rbx_attn_mfma.hip, rbx_attn_stream.h, rbx_attn_planes.h) through ops.attention,
ops.attention_packed, ops.attention_dropout_mask and, where a form or an output is only reachable below them (lse, a NULL
lse buffer, row pitches wider than E), the C entry points: forward output, lse, returned probabilities and dQ, dK, dV for a
fixed random cotangent, every element against the float64 restatement of oracle/attn64.py with
|got - want| <= C eps32 A + tiny (C per form as derived there, A = 0 means exactly zero).  Every case names the form that
oracle.attn64.attn_form says it reaches and asserts it first: a moved dispatch threshold fails the table, not the arithmetic.

Inputs per form (oracle.attn64.make_inputs): randn; scores up to +-60 with the row maximum on the first key, on the last
key, or rising along the keys (on the diagonal of a causal row: the running maximum moves at every step); near one-hot
rows; for the hd-32 split forms also peaks of 200, so that one half of a heavy tile leads the other by more than
log(FLT_MAX) = 88; masks that hide random entries, a 32-key tile, a whole LDS chunk of keys (the first or the last), and
every key of every third row, with both fills; dropout at
p = 0.1 and 0.5 with the kernel's own keep mask injected into the restatement.

Rows that the mask hides entirely.  mask_fill = -1e9: uniform over the causally visible keys, forward and backward, and
nothing flows back into q and k through the replaced scores (torch's masked_fill chain).  mask_fill = -inf: o and the
visible probabilities of the row are NaN and lse is -inf, as torch gives; dV is NaN at every key the row sees (all of
them, or j <= i with ``causal``), dQ of the row and its share of dK are zero, as masked_fill's backward gives.  Two differences from torch are pinned, not changed: with
``causal`` the causally hidden entries of such a row come back as 0, not NaN (the kernel never touches them; the row's o is
NaN either way, which is what a model sees), and nn.MultiheadAttention, which ADDS a float mask instead of masked_fill,
would also make dQ and dK NaN -- SASRec's causal mask is the ``causal`` flag here, it hides no row entirely.

split == 1 of attn_mfma_fwd_kernel (looping AND split) is unreachable from run_fwd: head_dim 32 never loops (the looping
branch is hd 64 only), at head_dim 64 causal nT 3 .. 7 goes to the streamed or planes kernel, nT = 8 needs
2 256 65 4 + 4 (2048 + 128) 4 = 167 936 bytes > 160 KB for the merge slots, and nT <= 2 does not split.  attn_form asserts
it for every L; the code is left alone.

The npf = 5 case (non-causal, hd 64, L 129 .. 160, more than 256 sequences: Lp = 160 runs the NPF = 8 instantiation):
correct.  prefetch_rows clamps the row of every float4 to L - 1, so the three extra loads per thread read row L - 1 again,
in bounds; commit_rows writes i < Lp 16 only, so they are never stored.  Wasteful (3 of 8 loads), not wrong; held to
float64 and to the per-sequence launches bit for bit below.

Fixed with this file (rbx_attn.hip, the VALU backward with an explicit mask; pinned by
test_rows_hidden_entirely_by_the_mask, whose four cases all fail on the parent commit's kernels, and by the chunk-0 case
of test_valu_three_chunks):
  * a row masked entirely with mask_fill = -1e9 has lse = -1e9 + log n, which float32 rounds to -1e9: attn_bwd_dkv_kernel
    recomputed p = exp(fill - lse) = 1 instead of 1 / n and dV came out n times too large (at -1e6 float32 keeps part of
    log n and p is off by a few per cent).  attn_bwd_dq_kernel, which walks the row anyway, now counts its masked keys
    and, where every visible key is masked and the fill is finite, leaves a NaN in the row's D slot (such a row has dS == 0
    everywhere, its D is never used); attn_bwd_dkv_kernel takes p = 1 / (visible keys) for a row flagged so, whatever the
    size of the fill (cases at -1e9, -1e6 and -30).
  * both backward kernels passed dS through masked entries into dQ and dK; masked_fill passes none.  Invisible where a row is
    only partly masked (p is 0 there), wrong in a row masked entirely.  dS is now zero at masked entries.
  * under ``causal`` both kernels walk keys a row does not see with p = 0 and formed dS = 0 * (dP - D) there; D of a row
    that -inf hides entirely is NaN, so dQ of that row and dK of the keys behind it came out NaN where masked_fill's
    backward gives finite values.  dS is now zero at unseen keys without the product.

Worst err / bound achieved on the MI355X (108 cases, 12 s; nothing above 0.03 of its bound, so nothing near 0.5; the
session ledger written by conftest holds every figure per test).  o / lse / p / dq / dk / dv:
  resident, unsplit (hd 32, 64)     0.012 / 0.013 / - / 0.0012 / 0.0028 / 0.0061       with dropout 0.0052 / 0.010 / - / 0.00094 / 0.0015 / 0.0038
  hd 32 split forward and backward  0.014 / 0.018 / - / 0.0017 / 0.0026 / 0.0058       with dropout 0.016 / 0.019 / - / 0.0014 / 0.0020 / 0.0062
  streamed ring, nT 3 .. 6          0.014 / 0.016 / - / 0.0012 / 0.0020 / 0.0058       with dropout 0.0039 / 0.0088 / - / 0.00068 / 0.00096 / 0.0028
  planes ring                       0.0078 / 0.011 / - / 0.00073 / 0.00088 / 0.0063    with dropout 0.0086 / 0.0069 / - / 0.0019 / 0.0015 / 0.0036
  planes ring, 515 sequences        0.0068 / 0.0073 / - / 0.00054 / 0.0017 / 0.0033    with dropout 0.0030 / 0.0054 / - / 0.00030 / 0.00061 / 0.0016
  looping, NPF 6, 7, 8 (and npf 5)  0.0073 / 0.012 / - / 0.0011 / 0.00065 / 0.0037     with dropout 0.0033 / 0.0066 / - / 0.00067 / 0.00034 / 0.0018
  packed operands                   0.013 / - / - / 0.00084 / 0.0022 / 0.0045
  VALU, chunks per hd               0.0093 / 0.011 / 0.010 / 0.0029 / 0.0036 / 0.0065  a chunk hidden 0.0059 / 0.0082 / 0.0086 / 0.00026 / 0.00077 / 0.0040
  VALU, three chunks                0.0041 / 0.0080 / 0.0028 / 0.00043 / 0.0015 / 0.0022  a chunk hidden 0.0032 / 0.0029 / 0.0067 / 0.00042 / 0.00027 / 0.0017
  VALU, query blocks, rectangles    0.018 / 0.024 / 0.013 / 0.0023 / 0.0042 / 0.0097   with dropout 0.019 / 0.022 / 0.013 / 0.0029 / 0.0057 / 0.0086
  MFMA shapes kept on the VALU      0.019 / 0.028 / 0.025 / 0.0023 / 0.0027 / 0.0083   (probabilities asked for: the backward is the MFMA one)
  rows hidden entirely              -1e9: 0.0087 / 0.012 / 0.015 / 0.0011 / 0.0028 / 0.0051   -1e6: 0.0058 / 0.0078 / 0.0077 / 0.0011 / 0.0015 / 0.0041
                                    -30: 0.0059 / 0.0086 / 0.010 / 0.0016 / 0.0017 / 0.0042   -inf: as -1e9, dV a NaN pattern
The forward sits at 1 to 3 per cent of its bound because C counts every dependent rounding of the chain at its worst case
while roundings average out, and because the large-score inputs put A_s (up to 200) into the relative weight of every
probability; dQ and dK sit lower still because A_dP and A_D are sums of absolute values where dP - D cancels.
Mutation check (three wrong variants of the attention sources in a scratch build, not kept; "before" are the 83 GPU tests
that existed before this file and are selected by -k "attention or attn or sasrec or sdpa"; this file has 108):
  (a) the forward's merge of two partial (m, l, O) triples rescales to its own maximum, not the larger    0 of 83 before, 6 of 108 here
      (every L of the hd-32 split test, on the "first200" input: o is not finite.  Up to +-60 the variant is the same
      softmax -- both partials are rescaled to one reference and exp(mo - m) stays below FLT_MAX -- which is why the
      peak-200 inputs are there)
  (b) attn_fwd_kernel skips the rescale of o at the first step of a chunk                                  4 of 83 before, 10 of 108 here
      (the chunk cases of every head_dim, three chunks, hd-64 MFMA shapes kept on the VALU kernel at L = 200 and 256, and
      the hidden-row cases with more than 184 keys)
  (c) attn_mfma_bwd_kv_kernel<32> drops the partner's share of SIMD 0's heavy tile from dK                 0 of 83 before, 8 of 108 here
      (every L of the hd-32 split test, the hd-32 L = 200 shape whose forward stays on the VALU, packed hd 32 L = 200)
"""
import ctypes

import pytest
import torch

from oracle import attn64 as A64
from test_attn64_restatement import make_mask
from test_gpu_interact_dims import Worst

pytestmark = pytest.mark.gpu
NEG_INF = float("-inf")
BIG_KINDS = ("first", "last", "ramp", "onehot")


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def hold(w, label, tag, got, want, A, C):
    """Worst.add, with the NaN / -inf pattern of ``want`` compared as a pattern first (nowhere else may one appear)."""
    got = got.detach().double().cpu().reshape(want.shape)
    special = torch.isnan(want) | torch.isinf(want)
    if bool(special.any()):
        assert torch.equal(torch.isnan(got), torch.isnan(want)), "%s: %s: NaN pattern differs" % (tag, label)
        inf = torch.isinf(want)
        assert torch.equal(got[inf], want[inf]), "%s: %s: -inf pattern differs" % (tag, label)
        got = torch.where(special, torch.zeros_like(got), got)
        want = torch.where(special, torch.zeros_like(want), want)
    w.add(label, tag, got, want, A, C)


def c_forward(q, k, v, mask, scale, causal, fill, p, seed, want_lse=True, want_probs=False):
    """rbx_attn_dropout_fwd / rbx_attn_fwd on [BH, L, hd] tensors: (o, lse, probs)."""
    from recbox_amd import ops
    from recbox_amd._lib import lib
    bh, lq, hd = q.shape
    lk = k.shape[1]
    o = torch.full_like(q, float("nan"))
    lse = torch.full((bh, lq), float("nan"), device=q.device) if want_lse else None
    pr = torch.full((bh, lq, lk), float("nan"), device=q.device) if want_probs else None
    if p:
        rc = lib.rbx_attn_dropout_fwd(P(q), P(k), P(v), P(mask), bh, lq, lk, hd, scale, int(causal), fill, p, seed,
                                      P(ops.dropout_tick(q.device)), P(o), P(lse), P(pr), None)
    else:
        rc = lib.rbx_attn_fwd(P(q), P(k), P(v), P(mask), bh, lq, lk, hd, scale, int(causal), fill, P(o), P(lse), P(pr), None)
    assert rc == 0
    torch.cuda.synchronize()
    return o, lse, pr


def run_ops(q, k, v, mask, scale, causal, fill, probs, p, seed, do):
    from recbox_amd import ops
    qq, kk, vv = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    o, pr = ops.attention(qq, kk, vv, mask=mask, scale=scale, causal=causal, fill=fill, need_probs=probs, dropout_p=p, seed=seed)
    o.backward(do)
    torch.cuda.synchronize()
    return o.detach(), pr, qq.grad, kk.grad, vv.grad


def sample_of(bh):
    """first, last and middle sequences and their neighbours; beyond 256 always the second trip and the final odd one"""
    if bh <= 12:
        return list(range(bh))
    return sorted(set(i for i in (0, 1, bh // 2 - 1, bh // 2, 255, 256, 257, bh - 2, bh - 1) if 0 <= i < bh))


def one_case(w, label, bh, lq, lk, hd, causal, kind, form, mkind=None, fill=-1e9, probs=False, p=0.0, seed=0, grads=True):
    from recbox_amd import ops
    f = A64.attn_form(bh, lq, lk, hd, causal, mkind is not None, probs)
    assert f == form, "dispatch table: (%d, %d, %d, %d, causal %s) is %s, the case says %s" % (bh, lq, lk, hd, causal, f, form)
    tag = "[%d, %d x %d, %d]%s %s %s%s p %g %s" % (bh, lq, lk, hd, " causal" if causal else "", kind, mkind or "",
                                                   " fill %g" % fill if mkind else "", p, "/".join(f))
    q, k, v, scale = A64.make_inputs(kind, bh, lq, lk, hd, seed)
    mask = make_mask(mkind, bh, lq, lk, seed + 1, chunk=A64.attn_chunk(lk, hd))
    do = torch.randn(bh, lq, hd, generator=torch.Generator().manual_seed(seed + 2))
    dev = [t.cuda() for t in (q, k, v)]
    mdev = None if mask is None else mask.cuda()
    dseed = 1234 + seed
    o, pr, dq, dk, dv = run_ops(dev[0], dev[1], dev[2], mdev, scale, causal, fill, probs, p, dseed, do.cuda())
    o2, lse, _ = c_forward(dev[0], dev[1], dev[2], mdev, scale, causal, fill, p, dseed, want_probs=probs)
    assert torch.equal(o.isnan(), o2.isnan()) and torch.equal(o.nan_to_num(0.0), o2.nan_to_num(0.0)), tag + ": C entry != ops"
    keep = ops.attention_dropout_mask(bh, lq, lk, p, dseed).cpu() if p else None
    idx = sample_of(bh)
    sel = (lambda t: None if t is None else t[idx])
    fw = A64.attn_fwd(sel(q), sel(k), sel(v), sel(mask), scale, causal, fill, sel(keep), p)
    cf, cb = A64.c_fwd(f, lk, hd), A64.c_bwd(f, lq, lk, hd)
    hold(w, label + " o", tag, o[idx], *fw["o"], cf)
    hold(w, label + " lse", tag, lse[idx], *fw["lse"], cf)
    if probs:
        hold(w, label + " p", tag, pr[idx], *fw["p"], cf)
    if grads:
        bw = A64.attn_bwd(sel(q), sel(k), sel(v), sel(mask), scale, causal, fill, sel(do), sel(keep), p)
        hold(w, label + " dq", tag, dq[idx], *bw["dq"], cb)
        hold(w, label + " dk", tag, dk[idx], *bw["dk"], cb)
        hold(w, label + " dv", tag, dv[idx], *bw["dv"], cb)
    return dev, do, (o, dq, dk, dv), dseed, scale


def in_launches(dev, do, whole, step, scale, causal, p, dseed):
    """the same sequences in launches of at most ``step`` (even: pairs keep their partners): bit for bit -- without dropout,
    whose mask is a function of the sequence's index in its launch"""
    bh = dev[0].shape[0]
    parts = [run_ops(dev[0][lo:lo + step], dev[1][lo:lo + step], dev[2][lo:lo + step], None, scale, causal, NEG_INF, False, 0.0,
                     dseed, do.cuda()[lo:lo + step]) for lo in range(0, bh, step)]
    for i, name in ((0, "o"), (2, "dq"), (3, "dk"), (4, "dv")):
        got = torch.cat([pp[i] for pp in parts])
        assert torch.equal(whole[(0, None, 1, 2, 3)[i]], got), name


def kinds_for(i, all_kinds):
    return ("randn",) + (BIG_KINDS if all_kinds else (BIG_KINDS[i % 4],))


# ---- matrix-core route ---------------------------------------------------------------------------------------------------
RES32 = [(L, c, 5) for L in (1, 31, 32, 33, 64) for c in (False, True)] + [(L, False, 5) for L in (65, 200, 255, 256)]
RES64 = [(L, c, 5) for L in (1, 33, 64) for c in (False, True)] + [(L, False, 5) for L in (65, 128, 200, 256)] + \
        [(225, True, 5), (256, True, 5)]


@pytest.mark.parametrize("hd,L,causal,bh", [(32,) + c for c in RES32] + [(64,) + c for c in RES64])
def test_resident_unsplit(hd, L, causal, bh):
    w = Worst()
    form = ("resident", "mfma:split" if causal and L > 64 else "mfma")
    for i, kind in enumerate(kinds_for(L, False)):
        one_case(w, "resident hd%d" % hd, bh, L, L, hd, causal, kind, form, seed=i)
    one_case(w, "resident hd%d dropout" % hd, bh, L, L, hd, causal, "randn", form, p=0.1 if L % 2 else 0.5, seed=9)
    w.close()


@pytest.mark.parametrize("L", [65, 96, 97, 200, 255, 256])
def test_head_dim_32_split_forward_and_split_backward(L):
    w = Worst()
    form = ("resident:split2", "mfma:split")
    # ("first200" / "last200": one half of a heavy tile leads the other by more than 88, so a merge that rescales to the
    #  smaller of the two maxima overflows)
    for i, kind in enumerate(kinds_for(L, True) + ("first200", "last200")):
        one_case(w, "split hd32", 5, L, L, 32, True, kind, form, seed=i)
    one_case(w, "split hd32 dropout", 5, L, L, 32, True, "ramp", form, p=0.5 if L % 2 else 0.1, seed=9)
    w.close()


@pytest.mark.parametrize("L,nT", [(65, 3), (97, 4), (128, 4), (129, 5), (160, 5), (161, 6), (192, 6)])
@pytest.mark.parametrize("bh", [2, 7])
def test_streamed_ring_each_block_shape(L, nT, bh):
    w = Worst()
    form = ("stream:%d" % nT, "mfma:split")
    for i, kind in enumerate(kinds_for(L + bh, bh == 7)):
        one_case(w, "stream nT%d" % nT, bh, L, L, 64, True, kind, form, seed=i)
    one_case(w, "stream nT%d dropout" % nT, bh, L, L, 64, True, "randn", form, p=0.1 if bh == 2 else 0.5, seed=9)
    w.close()


@pytest.mark.parametrize("L", [193, 200, 224])
def test_planes_ring(L):
    w = Worst()
    form = ("planes", "mfma:split")
    for i, kind in enumerate(kinds_for(L, True)):
        one_case(w, "planes", 5, L, L, 64, True, kind, form, seed=i)
    one_case(w, "planes dropout", 5, L, L, 64, True, "last", form, p=0.1 if L % 2 else 0.5, seed=9)
    w.close()


@pytest.mark.parametrize("L,kind", [(193, "randn"), (200, "ramp"), (224, "last")])
def test_planes_ring_with_more_pairs_than_workgroups(L, kind):
    """515 sequences are 258 pairs on 256 workgroups: two workgroups take a second pair, the last pair holds one sequence."""
    w = Worst()
    form = ("planes:loop", "mfma:split")
    dev, do, whole, dseed, scale = one_case(w, "planes loop", 515, L, L, 64, True, kind, form, seed=1)
    in_launches(dev, do, whole, 256, scale, True, 0.0, dseed)
    if L == 200:
        one_case(w, "planes loop dropout", 515, L, L, 64, True, "randn", form, p=0.5, seed=9)
    w.close()


LOOP = [(L, False) for L in (129, 160, 161, 192, 193, 224, 225, 256)] + [(225, True), (256, True)]


@pytest.mark.parametrize("L,causal", LOOP)
@pytest.mark.parametrize("bh,kind", [(257, "randn"), (300, "last")])
def test_looping_forward_each_prefetch_count(L, causal, bh, kind):
    """More than 256 sequences and Lp >= 160 at head_dim 64: one workgroup per CU loops and prefetches.  L = 129 and 160 are the
    npf = 5 case on the NPF = 8 body.  Sampled sequences (the second trip and the last one among them) against float64, all
    of them bit for bit against launches of at most 256, which take the one-workgroup-per-sequence kernel."""
    w = Worst()
    Lp = -(-L // 32) * 32
    npf = Lp // 32
    form = ("loop:%d" % (npf if npf in (6, 7) else 8), "mfma:split" if causal else "mfma")
    dev, do, whole, dseed, scale = one_case(w, "loop NPF%s" % form[0][5:], bh, L, L, 64, causal, kind, form, seed=2)
    assert A64.attn_form(150, L, L, 64, causal, False, False).fwd == "resident"
    in_launches(dev, do, whole, 150, scale, causal, 0.0, dseed)
    if bh == 257:
        one_case(w, "loop dropout", bh, L, L, 64, causal, "randn", form, p=0.1 if causal else 0.5, seed=9)
    w.close()


# ---- VALU route ----------------------------------------------------------------------------------------------------------
CHUNK = {4: 2456, 8: 1360, 16: 720, 32: 368, 64: 184}


@pytest.mark.parametrize("hd", [4, 8, 16, 32, 64])
def test_valu_chunks_of_keys_and_of_queries(hd):
    C = CHUNK[hd]
    assert A64.attn_chunk(10 ** 6, hd) == C
    w = Worst()
    bh = 1 if hd <= 8 else 2
    # one chunk; exactly one chunk; C + 9 keys for a few queries; C + 1 square: the one-row last chunk, over the queries too
    one_case(w, "valu hd%d" % hd, 3, 37, 37, hd, True, "randn", ("valu:1", "valu:1,1"), mkind="random", seed=1)
    one_case(w, "valu hd%d" % hd, bh, 9, C, hd, False, "last", ("valu:1", "valu:1,1"), mkind="random", seed=2)
    one_case(w, "valu hd%d" % hd, bh, 9, C + 9, hd, False, "last", ("valu:2", "valu:2,1"), mkind="random", seed=3)
    one_case(w, "valu hd%d" % hd, bh, 9, C + 9, hd, True, "first", ("valu:2", "valu:2,1"), mkind="tile", seed=4)
    # a mask that hides a whole chunk of keys: the first (the running maximum starts at the fill), the last
    one_case(w, "valu hd%d chunk hidden" % hd, bh, 9, C + 9, hd, False, "first", ("valu:2", "valu:2,1"), mkind="chunk0", seed=10)
    one_case(w, "valu hd%d chunk hidden" % hd, bh, 9, C + 9, hd, False, "last", ("valu:2", "valu:2,1"), mkind="chunklast",
             fill=NEG_INF, probs=True, seed=11)
    # (hd 4 and 8 keep two of the four square runs: the float64 side of 2457 x 2457 scores is what takes the time)
    for i, kind in enumerate(("ramp", "randn", "last") if hd >= 16 else ("ramp",)):
        one_case(w, "valu hd%d square" % hd, bh, C + 1, C + 1, hd, True, kind, ("valu:2", "valu:2,2"), mkind="random",
                 probs=kind == "ramp", seed=5 + i)
    if hd >= 16:
        one_case(w, "valu hd%d square" % hd, bh, C + 1, C + 1, hd, False, "first", ("valu:2", "valu:2,2"), mkind="random", seed=8)
    one_case(w, "valu hd%d dropout" % hd, bh, C + 1, C + 1, hd, True, "randn", ("valu:2", "valu:2,2"), mkind="random", p=0.5,
             probs=True, seed=9)
    w.close()


def test_valu_three_chunks():
    w = Worst()
    for i, (causal, kind) in enumerate(((True, "ramp"), (False, "last"), (True, "randn"))):
        one_case(w, "valu 3 chunks", 2, 400, 400, 64, causal, kind, ("valu:3", "valu:3,3"), mkind="random", probs=i == 2, seed=i)
    one_case(w, "valu 3 chunks", 2, 400, 400, 64, True, "first", ("valu:3", "valu:3,3"), mkind="tile", seed=4)
    # a whole chunk hidden: chunk 0 under ``causal`` hides rows 0 .. 183 entirely (uniform at -1e9); the last chunk at -inf
    one_case(w, "valu 3 chunks, chunk hidden", 2, 400, 400, 64, True, "ramp", ("valu:3", "valu:3,3"), mkind="chunk0", probs=True,
             seed=6)
    one_case(w, "valu 3 chunks, chunk hidden", 2, 400, 400, 64, False, "last", ("valu:3", "valu:3,3"), mkind="chunklast",
             fill=NEG_INF, seed=7)
    one_case(w, "valu 3 chunks, chunk hidden", 2, 400, 400, 64, True, "randn", ("valu:3", "valu:3,3"), mkind="chunklast",
             p=0.5, seed=8)
    one_case(w, "valu 3 chunks dropout", 2, 399, 401, 64, True, "randn", ("valu:3", "valu:3,3"), mkind="random", p=0.1,
             probs=True, seed=5)
    w.close()


@pytest.mark.parametrize("lq,lk,hd", [(1, 40, 16), (255, 40, 16), (256, 40, 16), (257, 40, 16), (513, 40, 16), (70, 300, 32),
                                      (300, 70, 32), (513, 513, 16), (13, 7, 8), (7, 13, 4)])
def test_valu_query_blocks_and_rectangles(lq, lk, hd):
    """one, two and three query blocks and a ragged last one; lq != lk both ways, causal: key j > i is hidden
    (torch.tril(ones(lq, lk)), which the restatement uses)."""
    w = Worst()
    nk, nq = -(-lk // A64.attn_chunk(lk, hd)), -(-lq // A64.attn_chunk(lq, hd))
    form = ("valu:%d" % nk, "valu:%d,%d" % (nk, nq))
    for i, (causal, kind) in enumerate(((True, "randn"), (True, "ramp"), (False, "last"), (True, "onehot"))):
        one_case(w, "valu rect", 3, lq, lk, hd, causal, kind, form, probs=i == 0, seed=i)
    one_case(w, "valu rect dropout", 3, lq, lk, hd, True, "randn", form, p=0.1, probs=True, seed=8)
    one_case(w, "valu rect dropout", 3, lq, lk, hd, False, "first", form, mkind="random", p=0.5, seed=9)
    w.close()


@pytest.mark.parametrize("hd,L,causal", [(64, 200, True), (64, 64, False), (32, 64, True), (32, 200, True), (64, 256, False)])
def test_matrix_core_shapes_kept_on_the_valu_kernels(hd, L, causal):
    """a mask, returned probabilities, both, or no lse buffer keep an MFMA shape on the VALU forward; without a mask the
    backward still runs on the matrix cores, from the VALU forward's o and lse"""
    w = Worst()
    nk = -(-L // A64.attn_chunk(L, hd))
    valu = "valu:%d" % nk
    mf = "mfma:split" if causal and L > 64 else "mfma"
    for i, kind in enumerate(("randn", "ramp")):
        one_case(w, "masked", 5, L, L, hd, causal, kind, (valu, "%s,%d" % (valu, nk)), mkind="random", seed=i)
        one_case(w, "probs, mfma backward", 5, L, L, hd, causal, kind, (valu, mf), probs=True, seed=2 + i)
        one_case(w, "masked, probs", 5, L, L, hd, causal, kind, (valu, "%s,%d" % (valu, nk)), mkind="tile", probs=True, seed=4 + i)
    one_case(w, "probs, mfma backward, dropout", 5, L, L, hd, causal, "randn", (valu, mf), probs=True, p=0.5, seed=7)
    # no lse buffer: only through the C entry point
    assert A64.attn_form(5, L, L, hd, causal, False, False, has_lse=False).fwd == valu
    q, k, v, scale = A64.make_inputs("last", 5, L, L, hd, 11)
    o, lse, _ = c_forward(q.cuda(), k.cuda(), v.cuda(), None, scale, causal, NEG_INF, 0.0, 0, want_lse=False)
    fw = A64.attn_fwd(q, k, v, None, scale, causal, NEG_INF)
    hold(w, "no lse buffer o", "[5, %d, %d]" % (L, hd), o, *fw["o"], A64.c_fwd(A64.Form(valu, ""), L, hd))
    w.close()


@pytest.mark.parametrize("lq,lk,hd", [(40, 40, 16), (200, 200, 64), (30, 50, 32), (257, 190, 64)])
def test_rows_hidden_entirely_by_the_mask(lq, lk, hd):
    """every third row masked entirely.  -1e9: uniform over the visible keys in the forward AND in the backward (fixed with
    this file: dV was n times too large, dQ and dK took gradients through the masked scores), also at a fill of -1e6, where
    float32 still holds part of log n.  -inf: the NaN pattern of the module docstring, gradients included: dV is NaN at the
    keys such a row sees (all of them, or j <= i with ``causal``), dQ and dK are finite."""
    w = Worst()
    nk, nq = -(-lk // A64.attn_chunk(lk, hd)), -(-lq // A64.attn_chunk(lq, hd))
    form = ("valu:%d" % nk, "valu:%d,%d" % (nk, nq))
    for causal in (False, True):
        for i, kind in enumerate(("randn", "first")):
            one_case(w, "hidden rows -1e9", 3, lq, lk, hd, causal, kind, form, mkind="rows", fill=-1e9, probs=True, seed=i)
            one_case(w, "hidden rows -inf", 3, lq, lk, hd, causal, kind, form, mkind="rows", fill=NEG_INF, probs=True, seed=i)
        one_case(w, "hidden rows -1e9 dropout", 3, lq, lk, hd, causal, "randn", form, mkind="rows", fill=-1e9, probs=True,
                 p=0.5, seed=5)
        one_case(w, "hidden rows -1e6", 3, lq, lk, hd, causal, "randn", form, mkind="rows", fill=-1e6, probs=True, seed=6)
        one_case(w, "hidden rows -30", 3, lq, lk, hd, causal, "randn", form, mkind="rows", fill=-30.0, probs=True, seed=7)
    w.close()


# ---- packed operands -----------------------------------------------------------------------------------------------------
def packed_c(q, kv, do, B, L, H, hd, scale, causal, pad):
    """rbx_attn_packed_* with Q, O, dO and dQ inside [B, L, E + pad] blocks and K | V, dK | dV the halves of [B, L, 2 E]."""
    from recbox_amd._lib import lib
    E = H * hd
    wide = lambda t: torch.cat([t, torch.full((B, L, pad), float("nan"), device=t.device)], -1).contiguous()   # noqa: E731
    qw, dow = wide(q), wide(do)
    ow, dqw = torch.full_like(qw, 7.0), torch.full_like(qw, 7.0)
    dkv = torch.full_like(kv, 7.0)
    lse = torch.empty(B * H, L, device=q.device)
    scratch = torch.empty(B * H, L, device=q.device)
    off = lambda t, n: ctypes.c_void_p(t.data_ptr() + 4 * n)                                                  # noqa: E731
    assert lib.rbx_attn_packed_fwd(P(qw), E + pad, P(kv), 2 * E, off(kv, E), 2 * E, B, H, L, hd, scale, int(causal), 0.0, 0,
                                   None, P(ow), E + pad, P(lse), None) == 0
    assert lib.rbx_attn_packed_bwd(P(qw), E + pad, P(kv), 2 * E, off(kv, E), 2 * E, P(ow), E + pad, P(dow), E + pad, P(lse),
                                   B, H, L, hd, scale, int(causal), 0.0, 0, None, P(dqw), E + pad, P(dkv), 2 * E,
                                   off(dkv, E), 2 * E, P(scratch), None) == 0
    torch.cuda.synchronize()
    assert bool((ow[..., E:] == 7.0).all()) and bool((dqw[..., E:] == 7.0).all()), "wrote between the rows"
    return ow[..., :E], dqw[..., :E], dkv


PACKED = [(32, 200, True, 3, 2, "resident:split2"), (64, 65, True, 3, 1, "stream:3"), (64, 128, True, 2, 2, "stream:4"),
          (64, 160, True, 3, 1, "stream:5"), (64, 192, True, 1, 4, "stream:6"), (64, 200, True, 3, 1, "planes"),
          (64, 256, True, 2, 2, "resident"), (64, 160, False, 65, 4, "loop:8"), (64, 200, False, 129, 2, "loop:7"),
          (32, 64, False, 2, 4, "resident"), (64, 200, True, 129, 4, "planes:loop")]


@pytest.mark.parametrize("hd,L,causal,B,H,fwd", PACKED)
def test_packed_operands_every_matrix_core_form(hd, L, causal, B, H, fwd):
    """ops.attention_packed and the C entry points at a wider pitch: bit-identical to the copying path through ops.attention,
    and the packed result itself against float64 (the pair must not be consistently wrong)."""
    from recbox_amd import ops
    E = H * hd
    assert A64.attn_form(B * H, L, L, hd, causal, False, False).fwd == fwd
    kind = "ramp" if causal else "last"
    q3, k3, v3, scale = A64.make_inputs(kind, B * H, L, L, hd, 3)
    pack = lambda t: t.view(B, H, L, hd).transpose(1, 2).reshape(B, L, E)                                      # noqa: E731
    q = pack(q3).cuda()
    kv = torch.cat([pack(k3), pack(v3)], -1).cuda()
    R3 = torch.randn(B * H, L, hd, generator=torch.Generator().manual_seed(4))
    R = pack(R3).cuda()
    for p in (0.0, 0.5):
        q1, kv1 = q.clone().requires_grad_(), kv.clone().requires_grad_()
        o1 = ops.attention_packed(q1, kv1, H, scale, causal=causal, dropout_p=p, seed=99)
        o1.backward(R)
        q2, kv2 = q.clone().requires_grad_(), kv.clone().requires_grad_()
        qh = q2.view(B, L, H, hd).transpose(1, 2)
        kh = kv2[..., :E].reshape(B, L, H, hd).transpose(1, 2)
        vh = kv2[..., E:].reshape(B, L, H, hd).transpose(1, 2)
        o2, _ = ops.attention(qh, kh, vh, scale=scale, causal=causal, fill=NEG_INF, dropout_p=p, seed=99)
        o2.transpose(1, 2).reshape(B, L, E).backward(R)
        assert torch.equal(o1.detach(), o2.detach().transpose(1, 2).reshape(B, L, E))
        assert torch.equal(q1.grad, q2.grad) and torch.equal(kv1.grad, kv2.grad)
        if p == 0.0:
            ow, dqw, dkvw = packed_c(q, kv, R, B, L, H, hd, scale, causal, pad=8)
            assert torch.equal(ow, o1.detach()) and torch.equal(dqw, q1.grad) and torch.equal(dkvw, kv1.grad)
            w = Worst()
            f = A64.attn_form(B * H, L, L, hd, causal, False, False)
            idx = sample_of(B * H)
            unpack = lambda t: t.detach().reshape(B, L, H, hd).transpose(1, 2).reshape(B * H, L, hd)[idx]        # noqa: E731
            fw = A64.attn_fwd(q3[idx], k3[idx], v3[idx], None, scale, causal, NEG_INF)
            bw = A64.attn_bwd(q3[idx], k3[idx], v3[idx], None, scale, causal, NEG_INF, R3[idx])
            cf, cb = A64.c_fwd(f, L, hd), A64.c_bwd(f, L, L, hd)
            tag = "packed [%d, %d, %d x %d] %s" % (B, L, H, hd, fwd)
            hold(w, "packed o", tag, unpack(o1), *fw["o"], cf)
            hold(w, "packed dq", tag, unpack(q1.grad), *bw["dq"], cb)
            hold(w, "packed dk", tag, unpack(kv1.grad[..., :E]), *bw["dk"], cb)
            hold(w, "packed dv", tag, unpack(kv1.grad[..., E:]), *bw["dv"], cb)
            w.close()
