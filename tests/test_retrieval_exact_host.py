"""CPU-only checks of tests/retrieval_exact.py, the restatements tests/test_gpu_retrieval_forms.py holds the integer
kernels to: topk_ref against torch.topk and hand-written rows, the case tables against the restated host loop of rbx_topk
(launch count, fast path or not, above or below the grid cap), the key encoding of the parent commit (why padding has to be
recognised by its position, and why the two zeros need one key), negsample_ref against the C oracle with a seed and an
offset above 2^32, and member_ref / penalize_ref / gather_ref on hand-written examples."""
import numpy as np
import pytest
import torch

import retrieval_exact as X
from oracle import c_oracle as C


def test_topk_ref_equals_torch_topk_on_tie_free_rows():
    for n, k in [(1, 1), (257, 64), (8193, 500), (20000, 1000)]:
        s = torch.stack([X.row_tie_free(n, k, seed) for seed in range(3)])
        assert len(torch.unique(s[0])) == n
        want = torch.topk(s, k, dim=1)
        vals, idx = X.topk_ref(s, k)
        assert torch.equal(vals, want.values) and torch.equal(idx, want.indices)
        remap = X.remap_ids(3, n, seed=n)
        assert torch.equal(X.topk_ref(s, k, remap)[1], torch.gather(remap, 1, want.indices))


def test_topk_ref_ties_zeros_padding_and_remap_by_hand():
    inf = float("inf")
    s = torch.tensor([[1.0, -0.0, 3.0, 0.0, 3.0, -inf, -X.FLT_MAX]])
    vals, idx = X.topk_ref(s, 9)
    assert idx.tolist() == [[2, 4, 0, 1, 3, 6, 5, -1, -1]]           # equal scores by ascending column; -0.0 == +0.0
    assert vals.tolist() == [[3.0, 3.0, 1.0, 0.0, 0.0, -X.FLT_MAX, -inf, -X.FLT_MAX, -X.FLT_MAX]]
    remap = torch.tensor([[70, 60, 50, 40, 30, 20, 2 ** 40 - 1]])
    assert X.topk_ref(s, 3, remap)[1].tolist() == [[50, 30, 70]]      # gathered on tied rows too
    vals, idx = X.topk_ref(torch.zeros(2, 0), 2)
    assert idx.tolist() == [[-1, -1]] * 2 and vals.tolist() == [[-X.FLT_MAX] * 2] * 2


def test_row_builders_are_what_they_say():
    n, k = 20000, 1000
    assert len(torch.unique(X.row_tie_free(n, k, 1))) == n
    assert len(torch.unique(X.row_quantised(n, k, 1))) == 16
    assert len(torch.unique(X.row_constant(n, k, 1))) == 1 and len(torch.unique(X.row_three_valued(n, k, 1))) == 3
    top = torch.topk(X.row_one_segment(n, k, 1), k).indices
    assert int(top.min()) // X.SEG == int(top.max()) // X.SEG
    # the sample of n = 20000 has stride 2 and 8 192 entries: positions from 16 384 on are never sampled
    assert X.sample_stride(n) == 2 and X.tail_start(n) == 16384 == X.SEG * X.sample_stride(n)
    assert int(torch.topk(X.row_tail_winners(n, k, 1), k).indices.min()) >= X.tail_start(n)
    half = X.row_half_one_value(n, k, 1)
    assert int((half == half[0]).sum()) >= n // 2
    z = X.row_zeros_mix(n, k, 1)
    signs = torch.signbit(z[z == 0])
    assert bool(signs.any()) and not bool(signs.all()) and int((z > 0).sum()) == 2 and int((z < 0).sum()) == 2
    assert int(torch.isinf(X.row_plus_inf(n, k, 1)).sum()) == 3
    for f in (0, 10, k - 1):
        r = X.row_neg_inf(n, f, 1)
        finite = torch.nonzero(torch.isfinite(r)).flatten()
        assert len(finite) == f and bool((r[~torch.isfinite(r)] == float("-inf")).all())
        if f >= 10:
            assert set((finite // X.SEG).tolist()) == set(range(X.nseg_of(n)))   # every segment has finite entries
    r = X.row_flt_max(257, 1000, 1)
    assert float(r[128]) == -X.FLT_MAX and float(r[0]) == float("-inf")
    assert torch.equal(X.build_rows(X.ROW_BUILDERS, 257, 1000)[-1], X.row_flt_max(257, 1000, 17 * len(X.ROW_BUILDERS)))
    assert X.build_rows(X.ROW_BUILDERS, 257, 64).shape == (len(X.ROW_BUILDERS), 257)


@pytest.mark.parametrize("group", sorted(X.TOPK_TABLES))
def test_case_tables_take_the_paths_they_name(group):
    for n, k, launches, fast in X.TOPK_TABLES[group]:
        X.check_topk_claim(n, k, launches, fast)


def test_named_boundaries_of_the_host_loop():
    assert X.sample_rank(16385, 1019) > 0 and X.sample_rank(16385, 1020) == 0       # the rank rule's boundary
    assert X.sample_rank(16384, 1) == 0 and X.sample_rank(20000, 1000) > 0
    assert X.levels(8192, 1024) == 1 and X.levels(8193, 1) == 2 and X.levels(16384, 1024) == 2
    assert X.levels(33000, 1024) == 2 and X.levels(70000, 500) == 2                 # the largest cases of the older tests
    assert X.levels(65537, 1024) == 3 and X.levels(524289, 1024) == 4
    # (65537, 1024): 9 segments -> 9 216 survivors -> 2 segments -> 2 048 survivors -> the sorting launch
    assert X.nseg_of(65537) == 9 and X.nseg_of(9 * 1024) == 2 and X.nseg_of(2 * 1024) == 1
    assert X.level_bytes(3, 8192, 7) == 0 and X.level_bytes(3, 8193, 7) == 3 * 2 * 7 * 12 + 256
    # a last segment shorter than k hands padding to the next level: 8193 -> 1 score, 8691 -> 499, 8692 -> 500 = k
    assert 8193 - X.SEG < 500 and 8691 - X.SEG == 499 and 8692 - X.SEG == 500 and 16400 - 2 * X.SEG < 64
    for rows, k, second_trip in X.MEMBER_SHAPES:
        assert (rows * k > X.GRID_CAP) == second_trip
    assert X.GRID_CAP == 1048576


def key_of_parent(v):
    """The key encoding of the parent commit: sign bit set -> all bits flipped, else the sign bit set."""
    u = np.asarray(v, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))


def key_of(v):
    """The encoding after the fix: -0.0 (0x80000000) takes the key of +0.0."""
    u = np.asarray(v, dtype=np.float32).view(np.uint32)
    return np.where(u > np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))


def test_key_model_shows_what_the_parent_got_wrong():
    ninf, pad = np.float32("-inf"), np.float32(-X.FLT_MAX)
    assert int(key_of_parent(pad)) == 0x00800000 and int(key_of_parent(ninf)) == 0x007FFFFF
    # the padding value outranks a real -inf: padding cannot be told from an element by its key, only by its position -1
    assert key_of_parent(pad) > key_of_parent(ninf) and key_of(pad) > key_of(ninf)
    # model of the level after a short segment under the parent: survivors = f finite + real -inf + padding words
    # (key << 32 | ~position, padding's ~(-1) = 0); the k best words hold padding although real -inf scores are left
    k, f = 500, 10
    real = X.row_neg_inf(8193, f, 0).numpy()
    seg0 = np.argsort(-real[:X.SEG], kind="stable")[:k]
    words = [(int(key_of_parent(real[p])) << 32) | (~int(p) & 0xFFFFFFFF) for p in list(seg0) + [8192]]
    words += [int(key_of_parent(pad)) << 32] * (k - 1)
    best = sorted(words, reverse=True)[:k]
    assert sum(1 for w in best if w & 0xFFFFFFFF == 0) == k - f
    assert X.topk_ref(torch.from_numpy(real)[None], k)[1].min() >= 0              # the restatement reports none
    # the two zeros are equal scores with different keys under the parent, one key after the fix
    assert int(key_of_parent(np.float32(0.0))) == 0x80000000 and int(key_of_parent(np.float32(-0.0))) == 0x7FFFFFFF
    assert key_of_parent(np.float32(0.0)) > key_of_parent(np.float32(-0.0))
    assert key_of(np.float32(0.0)) == key_of(np.float32(-0.0))
    # and the fixed encoding is still order-preserving on everything else
    v = np.array([-np.inf, -X.FLT_MAX, -3.0, -1e-45, 0.0, 1e-45, 2.5, X.FLT_MAX, np.inf], dtype=np.float32)
    assert (np.diff(key_of(v).astype(np.int64)) > 0).all()
    z = X.row_zeros_mix(64, 8, 4)
    order = np.argsort(-key_of_parent(z.numpy()).astype(np.int64), kind="stable")[:8]
    assert order.tolist() != X.topk_ref(z[None], 8)[1][0].tolist()               # the parent's order is not a stable sort


def test_negsample_ref_equals_the_c_oracle_on_high_words():
    seed, offset = 2 ** 40 + 3, 2 ** 32 + 7
    n_items, rows, negs = 1000, 40, 5
    pos = np.arange(rows, dtype=np.int64) * 3
    want = C.negsample(n_items, rows, negs, seed, offset, pos=pos)
    got, status = X.negsample_ref(n_items, rows, negs, seed, offset, pos=pos)
    assert status == 0 and (got == want).all()
    # the high words matter: dropping either changes the block
    assert not (C.negsample(n_items, rows, negs, seed & 0xFFFFFFFF, offset, pos=pos) == want).all()
    assert not (C.negsample(n_items, rows, negs, seed, offset & 0xFFFFFFFF, pos=pos) == want).all()
    # exclusion: an empty list, one item, 300 items, and all items but one (64 rejections, then the exact draw)
    lists = [[], [17], list(range(0, 900, 3)), [i for i in range(n_items) if i != 421]]
    off, items = X.make_csr(lists)
    query = np.arange(rows, dtype=np.int64) % 4
    want = C.negsample(n_items, rows, negs, seed, offset, query=query, excl_offsets=off, excl_items=items)
    got, status = X.negsample_ref(n_items, rows, negs, seed, offset, query=query, excl_offsets=off, excl_items=items)
    assert status == 0 and (got == want).all()
    assert (got[query == 3] == 421).all()
    for q in range(4):
        assert not np.isin(got[query == q], lists[q]).any()
    # a query outside the CSR: flagged, drawn unexcluded
    query[5], query[6] = -1, 4
    got, status = X.negsample_ref(n_items, rows, negs, seed, offset, query=query, excl_offsets=off, excl_items=items)
    plain = C.negsample(n_items, rows, negs, seed, offset)
    assert status == 1 and (got[5:7] == plain[5:7]).all() and (got[7:] == want[7:]).all()


def test_negsample_ref_philox_known_answer():
    # Random123 known-answer vector of Philox4x32-10 (counter and key of all ones)
    out = C.philox4x32_10([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2)
    assert [int(x) for x in out] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    assert X._draw(0, 0, 0, 1) == 0 and 0 <= X._draw(2 ** 63, 3, 2 ** 63 + 11, 2 ** 40) < 2 ** 40


def test_member_penalize_and_gather_refs_by_hand():
    off, items = X.make_csr([[5, 2 ** 40, 9], [], [7]])
    assert off.tolist() == [0, 3, 3, 4] and items.tolist() == [5, 9, 2 ** 40, 7]
    cand = np.array([[5, 6, -1, 2 ** 40], [5, 7, 9, -1], [7, 5, 2 ** 40, 0]], dtype=np.int64)
    query = np.array([0, 1, 2], dtype=np.int64)
    want = [[True, False, False, True], [False] * 4, [True, False, False, False]]
    assert X.member_ref(cand, query, off, items).tolist() == want
    s = np.array([[1.0, 2.0, 3.0, np.inf], [-0.0, 1.0, 2.0, 3.0], [0.25, -np.inf, 5.0, 6.0]], dtype=np.float32)
    out = X.penalize_ref(s, cand, query, off, items, -1e9)
    assert out.dtype == np.float32
    assert out[0].tolist() == [float(np.float32(1.0 - 1e9)), 2.0, 3.0, np.inf]
    assert out[1].view(np.uint32).tolist() == s[1].view(np.uint32).tolist()      # -0.0 keeps its sign on a non-member
    assert out[2].tolist() == [float(np.float32(0.25 - 1e9)), -np.inf, 5.0, 6.0]
    src = np.arange(12, dtype=np.uint8)
    got, status = X.gather_ref(src, 3, [3, 0, 0, 2])
    assert status == 0 and got.tolist() == [[9, 10, 11], [0, 1, 2], [0, 1, 2], [6, 7, 8]]
    got, status = X.gather_ref(src, 3, [1, -1, 4])
    assert status == 1 and got.tolist() == [[3, 4, 5], [0, 1, 2], [0, 1, 2]]
    assert [X.copy_unit(0, 0, b) for b in (1, 2, 6, 12, 16, 24, 48, 400)] == [1, 2, 2, 4, 16, 8, 16, 16]
    assert X.copy_unit(256 + 8, 256, 48) == 8 and X.copy_unit(256, 256 + 1, 48) == 1 and X.copy_unit(4, 2, 400) == 2
