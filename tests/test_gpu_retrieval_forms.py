"""The integer kernels of the retrieval and loader path through the C ABI, at every form they dispatch, against the
exact restatements of tests/retrieval_exact.py.  Every comparison is torch.equal or ==: there are no tolerances.
Outputs sit inside sentinel-filled blocks whose guards must come back intact; the top-k workspace is followed by 256
sentinel bytes.

rbx_topk (csrc/rbx_topk.hip, rbx_topk.h) -- every case stacks rows of different builders (tie-free, 16 levels, constant,
three-valued, winners in one segment, winners on the unsampled tail, half the row one value, +-0.0, +inf; a real
-FLT_MAX and -inf where k > n) in one call; each table entry names its launch count and whether the sampled-threshold
fast path applies, and the test asserts both (restated host loop, reported workspace size):
  * one level (n <= 8192: NULL workspace), n = 1, k > n, k = 1, k = 1024, k not a power of two, n = 8192 exactly
  * two levels without the fast path: last segment of 1, of k - 1 and of k scores, n = 16384 exactly, the rank rule's
    boundary (16385, 1020) -- and (16385, 1019) on the other side of it, fast
  * the fast path beside its fallbacks (ties, one-segment and unsampled-tail rows fall back on the device)
  * three and four exact levels: a non-final level reading a previous level's survivors, both survivor buffers reused
  * row_stride = n + 5 with and without d_index (ids below 2^40, compared on tied rows too); ops.topk on a column slice
  * rows of -inf with f < k finite scores, after a segment shorter than k: no padding among the results, no index read
    outside the row; k > n: (-FLT_MAX, -1) after every real entry, a real -FLT_MAX and a real -inf included
  * +0.0 and -0.0 are equal scores: the lower index first
  * rows = 0, n = 0, two runs with equal bits, and the refusals (k = 0, k = 1025, row_stride < n, NULL output, a workspace
    one byte short) with every sentinel intact
rbx_membership / rbx_penalize_members -- (rows, k) from (1, 1) to (1100, 1000), the last above the grid cap of 1 048 576
  elements (a second trip of the grid-stride loop); lists of 0, 1 and 300 ids up to 2^40; candidates -1, below the
  first entry, above the last, the first and the last; the penalty bit for bit, +-inf and -0.0 included
rbx_negsample(_checked) -- against the C oracle and, on the first 256 draws, Philox in Python integers: 1 200 000 draws
  (above the cap), seed 2^63 + 11, an offset whose block straddles 2^32, num_items 1, 2 and 2^40, num_negs = 0 with pos,
  pos NULL, a CSR with an empty list, a list of one item and a list of all items but one, queries outside the CSR
rbx_gather_rows -- source and destination bases at offsets 0, 1, 2, 4, 8 of a byte buffer x row_bytes 1 .. 400 (every copy
  unit reached through the base as well as through the row size), four columns of units 16, 4, 1 and 8 in one launch with
  more than 1 048 576 units, 64 columns (65 refused), the status word, a NULL status pointer, two runs with equal bits."""
import numpy as np
import pytest
import torch

import retrieval_exact as X
from oracle import c_oracle as C

pytestmark = pytest.mark.gpu

GUARD = 64                      # elements of sentinel before and after every output block
GAP = 3.0e38                    # scores between n and row_stride: they would win if they were read


def L():
    from recbox_amd import _lib
    return _lib


class Guarded(object):
    """`count` elements on the device between two guards, everything filled with a sentinel."""

    def __init__(self, count, dtype, sentinel):
        self.count, self.sentinel = count, sentinel
        self.buf = torch.full((count + 2 * GUARD,), sentinel, dtype=dtype, device="cuda")

    @property
    def ptr(self):
        return self.buf.data_ptr() + GUARD * self.buf.element_size()

    @property
    def body(self):
        return self.buf[GUARD:GUARD + self.count]

    def guards_intact(self):
        return bool((self.buf[:GUARD] == self.sentinel).all()) and bool((self.buf[GUARD + self.count:] == self.sentinel).all())

    def untouched(self):
        return bool((self.buf == self.sentinel).all())


def dev(a, dtype=None):
    t = torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a)
    return (t.to(dtype) if dtype is not None else t).cuda().contiguous()


# ---- rbx_topk ---------------------------------------------------------------------------------------------------------
def run_topk(scores, k, stride=None, index=None):
    """rbx_topk on scores [rows, n] (CPU) laid out at row_stride `stride`; -> (values, indexes) on the CPU, the reported
    workspace size.  Checks the return code, the guards of both outputs and the 256 bytes behind the workspace."""
    lib = L().lib
    rows, n = scores.shape
    stride = n if stride is None else stride
    d_scores = torch.full((rows, stride), GAP, device="cuda")
    d_scores[:, :n] = scores.cuda()
    d_index = None
    if index is not None:
        d_index = torch.full((rows, stride), -555, dtype=torch.int64, device="cuda")
        d_index[:, :n] = index.cuda()
    ov, oi = Guarded(rows * k, torch.float32, 12345.0), Guarded(rows * k, torch.int64, -777)
    ws_bytes = lib.rbx_topk_workspace_size(rows, n, k)
    ws = torch.full((ws_bytes + 256,), 0xA5, dtype=torch.uint8, device="cuda") if ws_bytes else None
    rc = lib.rbx_topk(d_scores.data_ptr() or None, None if d_index is None else d_index.data_ptr(), rows, n, stride, k,
                      ov.ptr, oi.ptr, None if ws is None else ws.data_ptr(), ws_bytes, None)
    torch.cuda.synchronize()
    assert rc == L().RBX_OK, L().last_error()
    assert ov.guards_intact() and oi.guards_intact()
    assert ws is None or bool((ws[ws_bytes:] == 0xA5).all())
    return ov.body.cpu().view(rows, k), oi.body.cpu().view(rows, k), ws_bytes


def check_topk(scores, n, k, launches, fast, stride=None, index=None):
    X.check_topk_claim(n, k, launches, fast)
    vals, idx, ws_bytes = run_topk(scores, k, stride, index)
    level = X.level_bytes(scores.shape[0], n, k)
    assert (level == 0) == (launches == 1)
    if fast:
        assert ws_bytes > 2 * level                     # the fast path's counters and candidate slots: it applies
    else:
        assert ws_bytes == 2 * level                    # 0 for one level: the workspace pointer was NULL
    want_vals, want_idx = X.topk_ref(scores, k, index)
    bad = torch.nonzero((idx != want_idx).any(1)).flatten().tolist()
    assert not bad, "rows %s: indexes differ from the stable sort (n=%d, k=%d)" % (bad, n, k)
    assert torch.equal(vals, want_vals)


def check_plain_and_remapped(builders, n, k, launches, fast):
    scores = X.build_rows(builders, n, k, seed=n + k)
    check_topk(scores, n, k, launches, fast)
    check_topk(scores, n, k, launches, fast, index=X.remap_ids(scores.shape[0], n, seed=n))


@pytest.mark.parametrize("n,k,launches,fast", X.TOPK_ONE_LEVEL)
def test_topk_one_level(n, k, launches, fast):
    check_plain_and_remapped(X.ROW_BUILDERS, n, k, launches, fast)


@pytest.mark.parametrize("n,k,launches,fast", X.TOPK_TWO_LEVELS)
def test_topk_two_levels_without_the_fast_path(n, k, launches, fast):
    check_plain_and_remapped(X.ROW_BUILDERS, n, k, launches, fast)


@pytest.mark.parametrize("n,k,launches,fast", X.TOPK_FAST)
def test_topk_fast_path_beside_its_fallbacks(n, k, launches, fast):
    check_plain_and_remapped(X.ROW_BUILDERS, n, k, launches, fast)


@pytest.mark.parametrize("n,k,launches,fast", X.TOPK_DEEP)
def test_topk_three_and_four_levels(n, k, launches, fast):
    """Tied rows overflow the candidate slots and take the exact path: 3 and 4 launches, the later non-final ones reading
    the survivors (and their positions) of the level before; the tie-free row beside them stays on the fast path."""
    scores = X.build_rows(X.TIED_BUILDERS + [X.row_tie_free], n, k, seed=n)
    check_topk(scores, n, k, launches, fast)


@pytest.mark.parametrize("with_index", [False, True])
@pytest.mark.parametrize("n,k,launches,fast", X.TOPK_STRIDED)
def test_topk_row_stride_above_n(n, k, launches, fast, with_index):
    builders = X.ROW_BUILDERS if n < 65537 else X.TIED_BUILDERS + [X.row_tie_free, X.row_zeros_mix]
    scores = X.build_rows(builders, n, k, seed=n + 1)
    index = X.remap_ids(scores.shape[0], n, seed=k) if with_index else None
    check_topk(scores, n, k, launches, fast, stride=n + 5, index=index)


@pytest.mark.parametrize("with_index", [False, True])
@pytest.mark.parametrize("n,k,launches,fast", X.TOPK_NEG_INF)
def test_topk_neg_inf_rows_after_a_short_segment(n, k, launches, fast, with_index):
    """Fewer than k scores above -inf: the finite ones, then -inf by ascending index.  Where the last segment is shorter
    than k its padding travels to the next level; it is not an element, so no result is (-FLT_MAX, 4294967295) and no
    remapped id is read from outside the row."""
    scores = torch.stack([X.row_neg_inf(n, f, seed=n + f) for f in (0, 10, k - 1)])
    index = X.remap_ids(3, n, seed=n + k) if with_index else None
    check_topk(scores, n, k, launches, fast, index=index)
    vals, idx, _ = run_topk(scores, k, index=index)
    assert int(idx.min()) >= 0 and bool((vals[:, k - 1] == float("-inf")).all())
    if index is not None:
        assert bool((idx < 2 ** 40).all())


@pytest.mark.parametrize("with_index", [False, True])
@pytest.mark.parametrize("n,k", [(2, 1024), (257, 1000), (1, 3)])
def test_topk_padding_comes_after_every_real_entry(n, k, with_index):
    scores = torch.stack([X.row_flt_max(n, k, 1), X.row_neg_inf(n, min(n, 1), 2), torch.full((n,), -X.FLT_MAX)])
    index = X.remap_ids(3, n, seed=k) if with_index else None
    check_topk(scores, n, k, 1, False, index=index)
    vals, idx, _ = run_topk(scores, k, index=index)
    assert bool((idx[:, :n] >= 0).all()) and bool((idx[:, n:] == -1).all()) and bool((vals[:, n:] == -X.FLT_MAX).all())
    assert float(vals[2, 0]) == -X.FLT_MAX and (with_index or idx[2, :n].tolist() == list(range(n)))


@pytest.mark.parametrize("n,k,launches,fast", X.TOPK_ZEROS)
def test_topk_signed_zeros_are_equal_scores(n, k, launches, fast):
    only = torch.where(torch.arange(n) % 3 == 0, torch.tensor(-0.0), torch.tensor(0.0))
    scores = torch.stack([X.row_zeros_mix(n, k, seed) for seed in (1, 2)] + [only, -only])
    check_topk(scores, n, k, launches, fast)
    _, idx, _ = run_topk(scores, k)
    assert idx[2].tolist() == list(range(k)) and idx[3].tolist() == list(range(k))


def test_ops_topk_reads_a_column_slice_in_place(monkeypatch):
    from recbox_amd import ops
    n, k, wide = 20000, 64, 20005
    block = torch.full((len(X.ROW_BUILDERS), wide), GAP)
    block[:, :n] = X.build_rows(X.ROW_BUILDERS, n, k, seed=9)
    d_block = block.cuda()
    real, seen = ops.lib.rbx_topk, []

    def spy(*args):
        seen.append((args[0].value, args[4]))
        return real(*args)

    monkeypatch.setattr(ops.lib, "rbx_topk", spy)
    vals, idx = ops.topk(d_block[:, :n], k)
    vals_c, idx_c = ops.topk(d_block[:, :n].contiguous(), k)
    assert seen[0] == (d_block.data_ptr(), wide) and seen[1][1] == n          # no copy: the slice's own memory and stride
    assert torch.equal(vals, vals_c) and torch.equal(idx, idx_c)
    want_vals, want_idx = X.topk_ref(block[:, :n], k)
    assert torch.equal(idx.cpu(), want_idx) and torch.equal(vals.cpu(), want_vals)


def test_topk_empty_shapes_repeatability_and_refusals():
    lib, M = L().lib, L()
    # n = 0: k slots of padding per row; rows = 0: nothing is written
    vals, idx, ws_bytes = run_topk(torch.zeros(3, 0), 5)
    assert ws_bytes == 0 and bool((idx == -1).all()) and bool((vals == -X.FLT_MAX).all())
    ov, oi = Guarded(64, torch.float32, 12345.0), Guarded(64, torch.int64, -777)
    assert lib.rbx_topk(None, None, 0, 100, 100, 5, ov.ptr, oi.ptr, None, 0, None) == M.RBX_OK
    # two runs, equal bits (the candidate order of the fast path depends on atomics; the result must not)
    n, k = 20000, 1000
    scores = X.build_rows(X.ROW_BUILDERS, n, k, seed=5)
    a, b = run_topk(scores, k), run_topk(scores, k)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])
    # refusals: the code, and nothing written
    d = scores.cuda()
    rows = d.shape[0]
    ws_bytes = lib.rbx_topk_workspace_size(rows, n, k)
    ws = torch.full((ws_bytes + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    ov, oi = Guarded(rows * 1025, torch.float32, 12345.0), Guarded(rows * 1025, torch.int64, -777)

    def call(k_=k, stride=n, out=ov.ptr, ws_ptr=ws.data_ptr(), nbytes=ws_bytes):
        return lib.rbx_topk(d.data_ptr(), None, rows, n, stride, k_, out, oi.ptr, ws_ptr, nbytes, None)

    assert call(k_=0) == M.RBX_ERR_UNSUPPORTED
    assert call(k_=1025) == M.RBX_ERR_UNSUPPORTED
    assert call(stride=n - 1) == M.RBX_ERR_INVALID
    assert call(out=None) == M.RBX_ERR_INVALID
    assert call(nbytes=ws_bytes - 1) == M.RBX_ERR_WORKSPACE and "workspace" in M.last_error()
    assert call(ws_ptr=None) == M.RBX_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert ov.untouched() and oi.untouched() and bool((ws == 0xA5).all())                 # nothing was launched


# ---- rbx_membership / rbx_penalize_members ------------------------------------------------------------------------------
def member_case(rows, k, seed):
    g = np.random.RandomState(seed)
    long_list = np.sort(g.permutation(np.unique(g.randint(10, 2 ** 40 - 10, 400, dtype=np.int64)))[:300])
    lists = [[], [2 ** 40 - 5], long_list.tolist(), [3, 2 ** 33 + 1]]
    off, items = X.make_csr(lists)
    query = g.randint(0, len(lists), rows).astype(np.int64)
    cand = np.empty((rows, k), dtype=np.int64)
    for r, q in enumerate(query.tolist()):
        own = lists[q]
        pool = [-1, 0, 5, 2 ** 40] + ([own[0] - 1, own[-1] + 1, own[0], own[-1]] + own[:40] if own else [])
        pool += g.randint(0, 2 ** 40, 8, dtype=np.int64).tolist()
        cand[r] = g.choice(np.array(pool, dtype=np.int64), k)
    return cand, query, off, items


@pytest.mark.parametrize("rows,k,second_trip", X.MEMBER_SHAPES)
def test_membership_and_penalty_forms(rows, k, second_trip):
    lib = L().lib
    assert (rows * k > X.GRID_CAP) == second_trip
    cand, query, off, items = member_case(rows, k, seed=rows + k)
    want = X.member_ref(cand, query, off, items)
    if rows * k >= 1000:
        assert want.any() and not want.all()
    if second_trip:
        assert want.reshape(-1)[X.GRID_CAP:].any()                          # hits that only the second trip can flag
    d = [dev(a) for a in (cand, query, off, items)]
    flags = Guarded(rows * k, torch.uint8, 0xEE)
    rc = lib.rbx_membership(d[0].data_ptr(), rows, k, d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), flags.ptr, None)
    torch.cuda.synchronize()
    assert rc == 0 and flags.guards_intact()
    assert (flags.body.cpu().numpy().reshape(rows, k) == want.astype(np.uint8)).all()
    g = np.random.RandomState(k)
    scores = g.randn(rows, k).astype(np.float32)
    special = g.randint(0, 8, (rows, k))
    scores[special == 0] = np.inf
    scores[special == 1] = -np.inf
    scores[special == 2] = -0.0
    ref = X.penalize_ref(scores, cand, query, off, items, -1e9)
    out = Guarded(rows * k, torch.float32, 12345.0)
    out.body.copy_(dev(scores).flatten())
    rc = lib.rbx_penalize_members(d[0].data_ptr(), rows, k, d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), -1e9, out.ptr,
                                  None)
    torch.cuda.synchronize()
    assert rc == 0 and out.guards_intact()
    assert (out.body.cpu().numpy().view(np.uint32) == ref.reshape(-1).view(np.uint32)).all()


def test_membership_empty_shapes_and_refusals():
    lib, M = L().lib, L()
    cand, query, off, items = member_case(4, 6, seed=1)
    d = [dev(a).data_ptr() for a in (cand, query, off, items)]
    flags, out = Guarded(24, torch.uint8, 0xEE), Guarded(24, torch.float32, 12345.0)
    assert lib.rbx_membership(d[0], 0, 6, d[1], d[2], d[3], flags.ptr, None) == M.RBX_OK           # rows = 0: a no-op
    assert lib.rbx_penalize_members(d[0], 0, 6, d[1], d[2], d[3], -1e9, out.ptr, None) == M.RBX_OK
    assert lib.rbx_membership(d[0], 4, 0, d[1], d[2], d[3], flags.ptr, None) == M.RBX_ERR_INVALID   # k = 0
    assert lib.rbx_penalize_members(d[0], 4, 0, d[1], d[2], d[3], -1e9, out.ptr, None) == M.RBX_ERR_INVALID
    assert lib.rbx_membership(d[0], -1, 6, d[1], d[2], d[3], flags.ptr, None) == M.RBX_ERR_INVALID
    for hole in range(4):
        args = list(d)
        args[hole] = None
        assert lib.rbx_membership(args[0], 4, 6, args[1], args[2], args[3], flags.ptr, None) == M.RBX_ERR_INVALID
        assert lib.rbx_penalize_members(args[0], 4, 6, args[1], args[2], args[3], -1e9, out.ptr, None) == M.RBX_ERR_INVALID
    assert lib.rbx_membership(d[0], 4, 6, d[1], d[2], d[3], None, None) == M.RBX_ERR_INVALID
    assert lib.rbx_penalize_members(d[0], 4, 6, d[1], d[2], d[3], -1e9, None, None) == M.RBX_ERR_INVALID
    torch.cuda.synchronize()
    assert flags.untouched() and out.untouched()


# ---- rbx_negsample / rbx_negsample_checked -----------------------------------------------------------------------------
def run_negsample(num_items, rows, negs, seed, offset, pos=None, query=None, off=None, items=None, checked=True,
                  n_queries=None):
    """-> (out [rows, width] numpy, status word or None).  The guards of the output must stay intact."""
    lib = L().lib
    width = negs + (1 if pos is not None else 0)
    d = [None if a is None else dev(a, torch.int64) for a in (pos, query, off, items)]
    p = [None if t is None else t.data_ptr() for t in d]
    out = Guarded(rows * width, torch.int64, -777)
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    if checked:
        n_queries = (len(off) - 1 if off is not None else 0) if n_queries is None else n_queries
        rc = lib.rbx_negsample_checked(num_items, rows, negs, seed, offset, p[0], p[1], p[2], p[3], n_queries,
                                       status.data_ptr(), out.ptr, None)
    else:
        rc = lib.rbx_negsample(num_items, rows, negs, seed, offset, p[0], p[1], p[2], p[3], out.ptr, None)
    torch.cuda.synchronize()
    assert rc == L().RBX_OK, L().last_error()
    assert out.guards_intact()
    return out.body.cpu().numpy().reshape(rows, width), int(status.item()) if checked else None


NEGSAMPLE_CASES = {
    # name: (num_items, rows, num_negs, seed, offset, with pos)
    "above the grid cap": (3706, 150000, 8, 2 ** 63 + 11, 2 ** 32 - 3, False),
    "seed with a high word": (3706, 300, 7, 2 ** 63 + 11, 0, True),
    "offset straddles 2^32": (3706, 300, 7, 3, 2 ** 32 - 3, True),
    "one item": (1, 100, 3, 2 ** 40 + 3, 2 ** 32 + 7, True),
    "two items": (2, 100, 3, 2 ** 40 + 3, 2 ** 32 + 7, False),
    "2^40 items": (2 ** 40, 300, 7, 2 ** 40 + 3, 2 ** 32 + 7, True),
    "no negatives, pos only": (50, 100, 0, 5, 0, True),
}


@pytest.mark.parametrize("name", sorted(NEGSAMPLE_CASES))
def test_negsample_forms(name):
    num_items, rows, negs, seed, offset, with_pos = NEGSAMPLE_CASES[name]
    assert (rows * (negs + with_pos) > X.GRID_CAP) == (name == "above the grid cap")
    pos = (np.arange(rows, dtype=np.int64) * 13) % num_items if with_pos else None
    want = C.negsample(num_items, rows, negs, seed, offset, pos=pos)
    for checked in (True, False):
        got, status = run_negsample(num_items, rows, negs, seed, offset, pos=pos, checked=checked)
        assert got.shape == want.shape and (got == want).all() and not status
    head = -(-256 // negs) if negs else rows                               # rows that hold the first 256 draws
    ref, _ = X.negsample_ref(num_items, head, negs, seed, offset, pos=pos)
    assert (got[:head] == ref).all()
    if negs:
        assert int(got[:, int(with_pos):].min()) >= 0 and int(got[:, int(with_pos):].max()) < num_items
    if num_items == 2 ** 40:
        assert int(got[:, 1:].max()) >= 2 ** 32                             # ids that need the high word of the product


def test_negsample_exclusion_lists_of_every_length():
    num_items, rows, negs, seed, offset = 50, 600, 5, 2 ** 40 + 3, 2 ** 32 + 7
    lists = [[], [17], [i for i in range(num_items) if i != 42], list(range(0, 50, 2))]
    off, items = X.make_csr(lists)
    query = np.arange(rows, dtype=np.int64) % len(lists)
    pos = np.arange(rows, dtype=np.int64) % num_items
    want = C.negsample(num_items, rows, negs, seed, offset, pos=pos, query=query, excl_offsets=off, excl_items=items)
    for checked in (True, False):
        got, status = run_negsample(num_items, rows, negs, seed, offset, pos, query, off, items, checked=checked)
        assert (got == want).all() and not status
    assert (got[query == 2][:, 1:] == 42).all()                             # 64 rejections, then the exact draw
    for q, own in enumerate(lists):
        assert not np.isin(got[query == q][:, 1:], own).any()
    head = -(-256 // negs)
    ref, status = X.negsample_ref(num_items, head, negs, seed, offset, pos, query, off, items)
    assert status == 0 and (got[:head] == ref).all()


def test_negsample_query_outside_the_csr_is_flagged_and_drawn_unexcluded():
    num_items, rows, negs, seed, offset = 50, 64, 5, 7, 2 ** 32 - 3
    lists = [[], [17], [i for i in range(num_items) if i != 42]]
    off, items = X.make_csr(lists)
    query = np.arange(rows, dtype=np.int64) % 3
    good = C.negsample(num_items, rows, negs, seed, offset, query=query, excl_offsets=off, excl_items=items)
    plain = C.negsample(num_items, rows, negs, seed, offset)
    bad = query.copy()
    bad[5], bad[20] = -1, 3                                                 # both were query 2: all items but one excluded
    assert query[5] == 2 and query[20] == 2
    got, status = run_negsample(num_items, rows, negs, seed, offset, None, bad, off, items, checked=True)
    want = good.copy()
    want[[5, 20]] = plain[[5, 20]]
    assert status == 1 and (got == want).all() and not (plain[[5, 20]] == good[[5, 20]]).all()
    ref, ref_status = X.negsample_ref(num_items, rows, negs, seed, offset, None, bad, off, items)
    assert ref_status == 1 and (got == ref).all()
    got, status = run_negsample(num_items, rows, negs, seed, offset, None, query, off, items, checked=True)
    assert status == 0 and (got == good).all()


def test_negsample_refusals():
    lib, M = L().lib, L()
    out = Guarded(64, torch.int64, -777)
    t = torch.zeros(8, dtype=torch.int64, device="cuda").data_ptr()
    assert lib.rbx_negsample(0, 4, 4, 1, 0, None, None, None, None, out.ptr, None) == M.RBX_ERR_INVALID      # num_items = 0
    assert lib.rbx_negsample(-5, 4, 4, 1, 0, None, None, None, None, out.ptr, None) == M.RBX_ERR_INVALID
    assert lib.rbx_negsample(10, 4, 4, 1, 0, None, t, t, None, out.ptr, None) == M.RBX_ERR_INVALID           # offsets, no items
    assert lib.rbx_negsample(10, 4, 4, 1, 0, None, t, None, t, out.ptr, None) == M.RBX_ERR_INVALID           # items, no offsets
    assert lib.rbx_negsample(10, 4, 4, 1, 0, None, None, t, t, out.ptr, None) == M.RBX_ERR_INVALID           # no query
    assert lib.rbx_negsample(10, 4, 4, 1, 0, None, None, None, None, None, None) == M.RBX_ERR_INVALID        # NULL output
    assert lib.rbx_negsample(10, 4, -1, 1, 0, None, None, None, None, out.ptr, None) == M.RBX_ERR_INVALID
    assert lib.rbx_negsample(10, 0, 4, 1, 0, None, None, None, None, out.ptr, None) == M.RBX_OK              # rows = 0
    assert lib.rbx_negsample(10, 4, 0, 1, 0, None, None, None, None, out.ptr, None) == M.RBX_OK              # width = 0
    torch.cuda.synchronize()
    assert out.untouched()


# ---- rbx_gather_rows -----------------------------------------------------------------------------------------------------
def columns(specs):
    arr = (L().rbx_rowcopy_t * len(specs))()
    for a, (src, dst, row_bytes) in zip(arr, specs):
        a.src, a.dst, a.row_bytes = src, dst, row_bytes
    return arr


def test_gather_rows_base_misalignment_reaches_every_unit():
    lib = L().lib
    offsets, sizes = (0, 1, 2, 4, 8), (1, 2, 6, 12, 16, 24, 48, 400)
    n_src, m, lead = 37, 53, 64
    region = ((lead + 16 + m * max(sizes) + 64 + 255) // 256) * 256
    g = torch.Generator().manual_seed(11)
    src = torch.randint(0, 256, (16 + n_src * max(sizes),), generator=g, dtype=torch.uint8)
    index = torch.randint(0, n_src, (m,), generator=g)
    index[0], index[1] = n_src - 1, 0
    d_src, d_index = src.cuda(), index.cuda()
    cases = [(so, do, rb) for so in offsets for do in offsets for rb in sizes]
    d_dst = torch.full((len(cases) * region,), 0xCD, dtype=torch.uint8, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert d_src.data_ptr() % 16 == 0 and d_dst.data_ptr() % 16 == 0
    units = {}
    for i, (so, do, rb) in enumerate(cases):
        sp, dp = d_src.data_ptr() + so, d_dst.data_ptr() + i * region + lead + do
        units[(so, do, rb)] = X.copy_unit(sp, dp, rb)
        assert lib.rbx_gather_rows(columns([(sp, dp, rb)]), 1, d_index.data_ptr(), m, n_src, status.data_ptr(), None) == 0
    torch.cuda.synchronize()
    # every unit is reached through the row size on aligned bases, and lowered by either base alone
    assert set(units.values()) == {1, 2, 4, 8, 16}
    assert [units[(0, 0, rb)] for rb in sizes] == [1, 2, 2, 4, 16, 8, 16, 16]
    assert [units[(so, 0, 400)] for so in offsets] == [16, 1, 2, 4, 8] == [units[(0, do, 400)] for do in offsets]
    got, src_np, index_np = d_dst.cpu().numpy(), src.numpy(), index.numpy()
    assert int(status.item()) == 0
    for i, (so, do, rb) in enumerate(cases):
        want, _ = X.gather_ref(src_np[so:so + n_src * rb], rb, index_np)
        block = got[i * region:(i + 1) * region]
        body = block[lead + do:lead + do + m * rb]
        assert (body == want.reshape(-1)).all(), "src+%d dst+%d row_bytes=%d" % (so, do, rb)
        assert (block[:lead + do] == 0xCD).all() and (block[lead + do + m * rb:] == 0xCD).all(), (so, do, rb)


def test_gather_rows_mixed_units_above_the_grid_cap_twice():
    lib = L().lib
    n_src, m = 100, 42000
    sizes = (400, 12, 3, 24)                       # units 16, 4, 1 and 8: the grid is sized by the widest column
    g = torch.Generator().manual_seed(12)
    srcs = [torch.randint(0, 256, (n_src * rb,), generator=g, dtype=torch.uint8) for rb in sizes]
    index = torch.randint(0, n_src, (m,), generator=g)
    d_srcs, d_index = [s.cuda() for s in srcs], index.cuda()
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    runs = []
    for status_ptr in (status.data_ptr(), None):   # a NULL status pointer is accepted
        dsts = [Guarded(m * rb, torch.uint8, 0xCD) for rb in sizes]
        cols = columns([(s.data_ptr(), d.ptr, rb) for s, d, rb in zip(d_srcs, dsts, sizes)])
        assert [X.copy_unit(c.src, c.dst, c.row_bytes) for c in cols] == [16, 4, 1, 8]
        assert m * (sizes[0] // 16) > X.GRID_CAP and m * (sizes[1] // 4) < X.GRID_CAP
        assert lib.rbx_gather_rows(cols, len(sizes), d_index.data_ptr(), m, n_src, status_ptr, None) == 0
        torch.cuda.synchronize()
        assert all(d.guards_intact() for d in dsts)
        runs.append([d.body.cpu() for d in dsts])
    assert int(status.item()) == 0
    for s, rb, a, b in zip(srcs, sizes, runs[0], runs[1]):
        want, _ = X.gather_ref(s.numpy(), rb, index.numpy())
        assert (a.numpy() == want.reshape(-1)).all() and torch.equal(a, b), rb


def test_gather_rows_column_limit_and_status_word():
    lib, M = L().lib, L()
    n_src, m, rb = 9, 33, 20
    g = torch.Generator().manual_seed(13)
    srcs = [torch.randint(0, 256, (n_src * rb,), generator=g, dtype=torch.uint8) for _ in range(X.MAX_COLUMNS + 1)]
    d_srcs = [s.cuda() for s in srcs]
    index = torch.randint(0, n_src, (m,), generator=g)
    d_index = index.cuda()
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    dsts = [Guarded(m * rb, torch.uint8, 0xCD) for _ in srcs]
    specs = [(s.data_ptr(), d.ptr, rb) for s, d in zip(d_srcs, dsts)]
    assert lib.rbx_gather_rows(columns(specs), 65, d_index.data_ptr(), m, n_src, status.data_ptr(), None) == M.RBX_ERR_INVALID
    assert lib.rbx_gather_rows(columns(specs), 0, d_index.data_ptr(), m, n_src, status.data_ptr(), None) == M.RBX_ERR_INVALID
    assert lib.rbx_gather_rows(columns(specs[:2]), 2, None, m, n_src, status.data_ptr(), None) == M.RBX_ERR_INVALID
    assert lib.rbx_gather_rows(columns([(None, dsts[0].ptr, rb)]), 1, d_index.data_ptr(), m, n_src, None, None) == M.RBX_ERR_INVALID
    assert lib.rbx_gather_rows(columns([specs[0][:2] + (0,)]), 1, d_index.data_ptr(), m, n_src, None, None) == M.RBX_ERR_INVALID
    assert lib.rbx_gather_rows(columns(specs[:2]), 2, d_index.data_ptr(), 0, n_src, None, None) == M.RBX_OK       # nothing to copy
    torch.cuda.synchronize()
    assert all(d.untouched() for d in dsts) and int(status.item()) == 0
    assert lib.rbx_gather_rows(columns(specs[:64]), 64, d_index.data_ptr(), m, n_src, status.data_ptr(), None) == M.RBX_OK
    torch.cuda.synchronize()
    assert int(status.item()) == 0 and dsts[64].untouched()
    for s, d in zip(srcs[:64], dsts[:64]):
        want, _ = X.gather_ref(s.numpy(), rb, index.numpy())
        assert d.guards_intact() and (d.body.cpu().numpy() == want.reshape(-1)).all()
    # an index of -1 or n_src_rows: row 0 is copied there, the flag is set and every other row stays right
    bad = index.clone()
    bad[3], bad[17] = -1, n_src
    outs = [Guarded(m * rb, torch.uint8, 0xCD) for _ in range(2)]
    specs = [(s.data_ptr(), d.ptr, rb) for s, d in zip(d_srcs, outs)]
    assert lib.rbx_gather_rows(columns(specs), 2, bad.cuda().data_ptr(), m, n_src, status.data_ptr(), None) == M.RBX_OK
    torch.cuda.synchronize()
    assert int(status.item()) == 1
    for s, d in zip(srcs, outs):
        want, flag = X.gather_ref(s.numpy(), rb, bad.numpy())
        assert flag == 1 and (want[3] == s.numpy()[:rb]).all() and (want[17] == s.numpy()[:rb]).all()
        assert d.guards_intact() and (d.body.cpu().numpy() == want.reshape(-1)).all()
