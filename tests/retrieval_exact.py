"""Exact restatements of the integer kernels of the retrieval and loader path (rbx_topk, rbx_membership,
rbx_penalize_members, rbx_negsample, rbx_gather_rows) and the builders of the rows and case tables their tests share.
Plain Python, numpy and torch on the CPU: a stable sort, Python sets, numpy indexing and Philox in Python integers.
Nothing here needs a tolerance.  Used by tests/test_retrieval_exact_host.py (CPU) and tests/test_gpu_retrieval_forms.py."""
import numpy as np
import torch

from oracle import c_oracle as C

FLT_MAX = float(np.finfo(np.float32).max)
SEG = 8192                     # kTopkSeg: scores per workgroup = survivors' segment of every level
MAX_K = 1024                   # kTopkMaxK
GRID_CAP = 256 * 16 * 256      # kCUs * 16 blocks of 256 threads: elements one trip of a grid-stride loop covers
MAX_ATTEMPTS = 64              # kMaxAttempts of rbx_sampler.hip
MAX_COLUMNS = 64               # RBX_MAX_FIELDS


# ---- the host loop of rbx_topk ------------------------------------------------------------------------------------
def sample_rank(n, k):
    """topk_sample_rank: rank among 8 192 strided samples, 0 = the sampled threshold (fast path) does not apply."""
    if n <= 2 * SEG:
        return 0
    r = (4 * k * SEG + n - 1) // n + 8
    return r if r < SEG // 4 else 0


def sample_stride(n):
    return n // SEG


def nseg_of(n):
    return (n + SEG - 1) // SEG if n > 0 else 1


def levels(n, k):
    """Launches of topk_kernel on the exact path: every level keeps k survivors per segment of 8 192 until one segment
    per row is left; the launch over that segment sorts and is counted too."""
    nseg, count = nseg_of(n), 1
    while nseg > 1:
        nseg = nseg_of(nseg * k)
        count += 1
    return count


def level_bytes(rows, n, k):
    """One of the two ping-pong survivor buffers (the first level is the largest); 0 for rows of one segment."""
    nseg = nseg_of(n)
    return rows * nseg * k * 12 + 256 if nseg > 1 else 0


# (n, k, launches on the exact path, fast path applies): the tables of tests/test_gpu_retrieval_forms.py.  The claims are
# asserted against levels() / sample_rank() on the CPU and against the workspace size the library reports on the GPU.
TOPK_ONE_LEVEL = [(1, 1, 1, False), (1, 3, 1, False), (2, 1024, 1, False), (255, 64, 1, False), (256, 256, 1, False),
                  (257, 1000, 1, False), (8191, 500, 1, False), (8192, 1, 1, False), (8192, 1024, 1, False)]
TOPK_TWO_LEVELS = [(8193, 1, 2, False), (8193, 500, 2, False), (8193, 1024, 2, False), (8691, 500, 2, False),
                   (8692, 500, 2, False), (16384, 1024, 2, False), (16385, 1020, 2, False)]
TOPK_FAST = [(16385, 1019, 2, True), (20000, 64, 2, True), (20000, 1000, 2, True)]
TOPK_DEEP = [(65537, 1024, 3, True), (524289, 1024, 4, True)]
TOPK_STRIDED = [(257, 1000, 1, False), (8193, 500, 2, False), (20000, 1000, 2, True), (65537, 1024, 3, True)]
# rows of -inf with f < k finite entries; (16400, 64): three segments, the last one (16 scores) shorter than k
TOPK_NEG_INF = [(8193, 500, 2, False), (8193, 1024, 2, False), (20000, 1000, 2, True), (16400, 64, 2, True)]
TOPK_ZEROS = [(8192, 1024, 1, False), (8193, 500, 2, False), (20000, 1000, 2, True), (65537, 1024, 3, True)]
TOPK_TABLES = {"one level": TOPK_ONE_LEVEL, "two levels": TOPK_TWO_LEVELS, "fast": TOPK_FAST, "deep": TOPK_DEEP,
               "strided": TOPK_STRIDED, "-inf": TOPK_NEG_INF, "zeros": TOPK_ZEROS}
# (rows, k, more than one trip of the grid-stride loop)
MEMBER_SHAPES = [(1, 1, False), (3, 1024, False), (257, 7, False), (1100, 1000, True)]


def check_topk_claim(n, k, launches, fast):
    assert 1 <= k <= MAX_K
    assert levels(n, k) == launches, "(%d, %d): %d launches, the table says %d" % (n, k, levels(n, k), launches)
    assert (sample_rank(n, k) > 0) == fast, "(%d, %d): sample rank %d, the table says fast=%s" % (n, k, sample_rank(n, k), fast)


# ---- restatements ----------------------------------------------------------------------------------------------------
def topk_ref(scores, k, index=None):
    """(values [rows, k] fp32, indexes [rows, k] int64) of a stable descending sort of fp32 scores [rows, n]: equal scores
    (+0.0 and -0.0 are equal) keep ascending column order.  index [rows, n] int64 replaces the column as the reported
    index, on every row.  k > n: (-FLT_MAX, -1) after the n real entries."""
    scores = torch.as_tensor(scores, dtype=torch.float32)
    rows, n = scores.shape
    kk = min(k, n)
    vals = torch.full((rows, k), -FLT_MAX, dtype=torch.float32)
    idx = torch.full((rows, k), -1, dtype=torch.int64)
    if kk > 0:
        order = torch.sort(scores, dim=1, descending=True, stable=True)
        vals[:, :kk] = order.values[:, :kk]
        cols = order.indices[:, :kk]
        idx[:, :kk] = cols if index is None else torch.gather(torch.as_tensor(index, dtype=torch.int64), 1, cols)
    return vals, idx


def _csr_sets(query, off, items):
    off, items = np.asarray(off).tolist(), np.asarray(items).tolist()
    lists = [set(items[off[q]:off[q + 1]]) for q in range(len(off) - 1)]
    return [lists[q] for q in np.asarray(query).tolist()]


def member_ref(cand, query, off, items):
    """flags[r, j] = cand[r, j] in the list of query[r] (Python sets; a negative candidate is never a member)."""
    cand = np.asarray(cand)
    sets = _csr_sets(query, off, items)
    out = [[c >= 0 and c in s for c in row] for row, s in zip(cand.tolist(), sets)]
    return np.array(out, dtype=bool).reshape(cand.shape)


def penalize_ref(scores, cand, query, off, items, penalty):
    """float32(float64(s) + penalty) on members; every other score keeps its bits."""
    scores = np.asarray(scores, dtype=np.float32)
    hit = member_ref(cand, query, off, items)
    out = scores.copy()
    out[hit] = (scores[hit].astype(np.float64) + np.float64(penalty)).astype(np.float32)
    return out


def gather_ref(src_bytes, row_bytes, index):
    """(dst bytes [len(index), row_bytes], status): numpy indexing on the byte view of a column; an index outside
    [0, n_rows) copies row 0 and sets the status."""
    table = np.asarray(src_bytes, dtype=np.uint8).reshape(-1, row_bytes)
    index = np.asarray(index, dtype=np.int64)
    bad = (index < 0) | (index >= table.shape[0])
    return table[np.where(bad, 0, index)], int(bad.any())


def copy_unit(src_ptr, dst_ptr, row_bytes):
    """Bytes a lane of gather_rows_kernel moves per step: the alignment src, dst and row_bytes share, 16 at most."""
    bits = src_ptr | dst_ptr | row_bytes
    for unit in (16, 8, 4, 2):
        if bits % unit == 0:
            return unit
    return 1


def _draw(element, attempt, seed, num_items):
    """High 64 bits of (64 random bits) x num_items; counter (element lo, element hi, attempt, 0), key (seed lo, hi)."""
    m = 0xFFFFFFFF
    o = C.philox4x32_10([element & m, (element >> 32) & m, attempt, 0], [seed & m, (seed >> 32) & m])
    r = (int(o[1]) << 32) | int(o[0])
    return (r * num_items) >> 64


def negsample_ref(num_items, rows, num_negs, seed, offset=0, pos=None, query=None, excl_offsets=None, excl_items=None,
                  n_queries=None):
    """(out [rows, width] int64, status) in Python integers, as the header comment of rbx_sampler.hip states it: element =
    offset + r * num_negs + j (mod 2^64); up to 64 rejection rounds against the sorted exclusion list of query[r], then
    ONE exact draw over the complement (attempt 64, uniform in [0, num_items - n_excl), stepped over the excluded ids).
    A query outside [0, n_queries) sets the status and draws unexcluded."""
    width = num_negs + (1 if pos is not None else 0)
    out = np.zeros((rows, width), dtype=np.int64)
    status = 0
    off = None if excl_offsets is None else np.asarray(excl_offsets).tolist()
    items = None if excl_items is None else np.asarray(excl_items).tolist()
    if off is not None and n_queries is None:
        n_queries = len(off) - 1
    for r in range(rows):
        if pos is not None:
            out[r, 0] = int(pos[r])
        excl = []
        if off is not None:
            q = int(query[r])
            if q < 0 or q >= n_queries:
                status |= 1 if num_negs > 0 else 0
            else:
                excl = items[off[q]:off[q + 1]]
        banned = set(excl)
        for j in range(num_negs):
            element = (offset + r * num_negs + j) & (2 ** 64 - 1)
            item, found = 0, False
            for a in range(MAX_ATTEMPTS):
                item = _draw(element, a, seed, num_items)
                if item not in banned:
                    found = True
                    break
            if not found and len(excl) < num_items:
                item = _draw(element, MAX_ATTEMPTS, seed, num_items - len(excl))
                for e in excl:
                    if e > item:
                        break
                    item += 1
            out[r, width - num_negs + j] = item
    return out, status


# ---- rows: every builder is seeded and takes the length ---------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _distinct(m, seed):
    """m distinct fp32 values of both signs in random order (exact in fp32: multiples of 0.5 below 2^23)."""
    return (torch.randperm(m, generator=_gen(seed)).float() - m // 2) * 0.5


def row_tie_free(n, k, seed):
    return _distinct(n, seed)


def row_quantised(n, k, seed):
    return torch.randint(0, 16, (n,), generator=_gen(seed)).float() - 8.0


def row_constant(n, k, seed):
    return torch.full((n,), 1.5)


def row_three_valued(n, k, seed):
    return (torch.arange(n) % 3).float()


def row_one_segment(n, k, seed):
    """Zeros, and min(2k, n) distinct positive values next to each other: every winner inside one segment."""
    row = torch.zeros(n)
    width = min(2 * k, n)
    start = min(5000, n - width)
    row[start:start + width] = torch.randperm(width, generator=_gen(seed)).float() + 1.0
    return row


def tail_start(n):
    """First position of the tail no strided sample reaches: 8192 * (n // 8192) (where that is the row's start or
    end: the last quarter of the row)."""
    start = SEG * (n // SEG)
    return start if 0 < start < n else n - max(1, n // 4)


def row_tail_winners(n, k, seed):
    """Distinct negative values, and distinct positive ones on the whole tail: the row's largest all lie there."""
    row = -1.0 - torch.randperm(n, generator=_gen(seed)).float()
    t = tail_start(n)
    row[t:] = torch.randperm(n - t, generator=_gen(seed + 1)).float() + 1.0
    return row


def row_half_one_value(n, k, seed):
    row = _distinct(n, seed)
    row[::2] = row[0]
    return row


def row_zeros_mix(n, k, seed):
    """+0.0 and -0.0 at random, and (from 8 scores on) two positive and two negative values among them."""
    row = torch.where(torch.rand(n, generator=_gen(seed)) < 0.5, torch.tensor(0.0), torch.tensor(-0.0))
    if n >= 8:
        where = torch.randperm(n, generator=_gen(seed + 1))[:4]
        row[where] = torch.tensor([2.0, 1.0, -1.0, -3.0])
    return row


def row_plus_inf(n, k, seed):
    row = _distinct(n, seed)
    row[[0, n // 2, n - 1]] = float("inf")
    return row


def row_neg_inf(n, f, seed):
    """-inf everywhere but f distinct finite values of both signs, spread over all segments (position n - 1 first)."""
    row = torch.full((n,), float("-inf"))
    if f > 0:
        where = n - 1 - (torch.arange(f) * n) // f
        row[where] = _distinct(f, seed)
    return row


def row_flt_max(n, k, seed):
    """For k > n: a real -FLT_MAX score (and, from 2 scores on, a real -inf): both come before the padding."""
    row = _distinct(n, seed)
    row[n // 2] = -FLT_MAX
    if n >= 2:
        row[0] = float("-inf")
    return row


ROW_BUILDERS = [row_tie_free, row_quantised, row_constant, row_three_valued, row_one_segment, row_tail_winners,
                row_half_one_value, row_zeros_mix, row_plus_inf]
TIED_BUILDERS = [row_constant, row_three_valued, row_quantised]


def build_rows(builders, n, k, seed=0):
    """[len(builders), n] fp32: one row per builder (row_flt_max joins when k > n)."""
    use = list(builders) + ([row_flt_max] if k > n else [])
    return torch.stack([b(n, k, seed + 17 * i) for i, b in enumerate(use)])


def remap_ids(rows, width, seed):
    """Caller-side ids: full 64-bit values below 2^40, repeated values allowed."""
    return torch.randint(0, 2 ** 40, (rows, width), generator=_gen(seed))


def make_csr(lists):
    """offsets, items (int64) of sorted lists."""
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    items = np.concatenate([np.asarray(sorted(x), dtype=np.int64) for x in lists]) if lists else np.zeros(0, np.int64)
    return off, items.astype(np.int64)
