"""CPU checks of the float64 restatement of the generic embedding lookup (oracle/embed64.py) that
tests/test_gpu_embed_dims.py compares the lookup's kernels with: it equals float64 autograd on a plain-torch composition
for every pool, it agrees with the C oracle (orc_embed_fwd / orc_embed_bwd, float32, sequential sums) inside that sum's
own rounding, and its per-element bound is sharp enough to catch one lost lookup, one lost chunk of 16 sorted lookups in
a 70 000-lookup row, and one lost history item at seq_len = 300.  The case builders of the GPU file live here."""
import numpy as np
import pytest
import torch

from oracle.embed64 import C_BOUND, EPS32, Lookup64, Table, assert_value_mask_is_safe, bound_ratio, embed64, forward_ratio

POOLED = ("SUM", "SUM_ID", "MEAN_ID", "MEAN_VALUE")


# ---- case builders (shared with the GPU file) ------------------------------------------------------------------------
def magnitudes(shape, gen, lo=0.05):
    """float32 values with |v| in [lo, 1] and a random sign."""
    v = lo + (1 - lo) * torch.rand(shape, generator=gen)
    return (v * (torch.randint(0, 2, shape, generator=gen) * 2 - 1)).float()


def make_table(V, D, gen, pad=None, zero_rows=(), value_mask_safe=False):
    w = magnitudes((V, D), gen)
    if value_mask_safe:                                  # MEAN_VALUE reads it: no row sum near zero
        near = w.double().sum(1).abs() <= 0.01
        w[near] = w[near].abs()
    for r in zero_rows:
        w[r] = 0
    if pad is not None:
        w[pad] = 0
    if value_mask_safe:
        assert_value_mask_is_safe(w)
    return w


def history(V, B, L, gen, lo=1, fill=0, empty_frac=0.0, masked_frac=0.0):
    """ids [B, L] in [lo, V), the tail of every history beyond a random length set to ``fill``; ``masked_frac`` of the
    remaining positions and ``empty_frac`` of whole samples set to ``fill`` too."""
    ids = torch.randint(lo, V, (B, L), generator=gen)
    lens = torch.randint(0, L + 1, (B,), generator=gen)
    ids[torch.arange(L)[None, :] >= lens[:, None]] = fill
    if masked_frac:
        ids[torch.rand(B, L, generator=gen) < masked_frac] = fill
    if empty_frac:
        ids[torch.rand(B, generator=gen) < empty_frac] = fill
    return ids


def spec(name, kind="categorical", table=None, pool="NONE", L=1, mask_id=None, eps=0.0):
    return dict(name=name, kind=kind, table=table, pool=pool, L=L, mask_id=mask_id, eps=eps)


def grid_case(D, B, seed, big=200000, L=6):
    """The plan of the dim grid: tables of 3, 300, 5000 (no padding row) and ``big`` rows; a one-id lookup of each of
    three of them, SUM / MEAN_ID / MEAN_VALUE histories that share the 300-row table (rows 5 and 17 all zeros and not
    the padding row: MEAN_VALUE must not count them), a SUM_ID and a CONCAT history over the 5000-row table, one numeric
    feature.  ~5 % of the one-id lookups name the padding row; histories are ragged (id 0 beyond their length)."""
    gen = torch.Generator().manual_seed(seed)
    tables = {"T3": (make_table(3, D, gen, pad=0), 0),
              "T300": (make_table(300, D, gen, pad=0, zero_rows=(5, 17), value_mask_safe=True), 0),
              "T5000": (make_table(5000, D, gen), None),
              "Tbig": (make_table(big, D, gen, pad=0), 0),
              "wn": (magnitudes((D,), gen), None)}
    specs = [spec("num", kind="numeric", table="wn"),
             spec("one_big", table="Tbig"),
             spec("one_3", table="T3"),
             spec("sum", table="T300", pool="SUM", L=L),
             spec("mean_id", table="T300", pool="MEAN_ID", L=L, mask_id=0, eps=1e-16),
             spec("sum_id", table="T5000", pool="SUM_ID", L=L, mask_id=0),
             spec("mean_value", table="T300", pool="MEAN_VALUE", L=L, eps=1e-12),
             spec("concat", table="T5000", pool="CONCAT", L=L),
             spec("one_5000", table="T5000")]
    cols = {"num": torch.rand(B, generator=gen, dtype=torch.float64) * 2 - 0.5}
    for name, V in (("one_big", big), ("one_3", 3), ("one_5000", 5000)):
        ids = torch.randint(1, V, (B,), generator=gen)
        ids[torch.rand(B, generator=gen) < 0.05] = 0
        cols[name] = ids
    cols["sum"] = history(300, B, L, gen)
    cols["mean_id"] = history(300, B, L, gen)
    cols["mean_value"] = history(300, B, L, gen)
    cols["sum_id"] = history(5000, B, L, gen)
    cols["concat"] = history(5000, B, L, gen)
    return specs, tables, cols


def widths(specs, tables):
    offs, off = [], 0
    for s in specs:
        D = 1 if s["kind"] == "dense" else tables[s["table"]][0].shape[-1]
        offs.append(off)
        off += D * (s["L"] if s["pool"] == "CONCAT" else 1)
    return offs, off


def lookups64(specs, tables, cols, offsets=None):
    """Lookup64 list over float64 ``Table``s (one object per table key); returns (lookups, {key: Table})."""
    t64 = {k: Table(w) for k, (w, _) in tables.items()}
    offs = offsets if offsets is not None else widths(specs, tables)[0]
    out = []
    for s, off in zip(specs, offs):
        if s["kind"] == "dense":
            out.append(Lookup64("dense", cols[s["name"]], out_off=off))
            continue
        w, pad = tables[s["table"]]
        out.append(Lookup64(s["kind"], cols[s["name"]], t64[s["table"]], dim=w.shape[-1], pool=s["pool"], seq_len=s["L"],
                            padding_idx=pad if s["kind"] == "categorical" else None, mask_id=s["mask_id"], eps=s["eps"],
                            out_off=off))
    return out, t64


def hot_row_batch(n, seed, L=1, V=1000):
    """ids [n // L, L] of the hot-row case: id 7 draws 70 % of the lookups and id 3 another 20 % (the recipe of
    test_hot_rows_with_nonzero_gradients_are_summed_by_several_workgroups), id 11 exactly 250 and id 13 exactly 100 of them
    (chains of a few chunks), the rest uniform over the other rows; and the sign of every sample's dY: +1 for the samples
    that look up id 7, so that its terms cannot cancel, random for the others."""
    gen = torch.Generator().manual_seed(seed)
    B = n // L
    u = torch.rand(B * L, generator=gen)
    ids = torch.randint(20, V, (B * L,), generator=gen)
    ids[u < 0.7] = 7
    ids[(u >= 0.7) & (u < 0.9)] = 3
    rest = (u >= 0.9).nonzero().view(-1)
    ids[rest[:250]] = 11
    ids[rest[250:350]] = 13
    ids = ids.view(B, L)
    sign = (torch.randint(0, 2, (B,), generator=gen) * 2 - 1).double()
    sign[(ids == 7).any(1)] = 1.0
    return ids, sign


def hot_row_dy(sign, D, gen):
    """dY [B, D] with |dY| in [0.05, 1] and one sign per sample."""
    return ((0.05 + 0.95 * torch.rand(sign.shape[0], D, generator=gen)).double() * sign[:, None]).float()


# ---- 1. the restatement is the autograd of a plain composition --------------------------------------------------------
def _composition(specs, tables, cols, dY):
    """float64 autograd over nn.functional.embedding + masks + sums; returns (out, {table key: grad})."""
    F = torch.nn.functional
    leaves = {k: w.double().clone().requires_grad_(True) for k, (w, _) in tables.items()}
    parts = []
    for s in specs:
        col = cols[s["name"]]
        if s["kind"] == "dense":
            parts.append(col.float().double().view(-1, 1))
            continue
        W, pad = leaves[s["table"]], tables[s["table"]][1]
        if s["kind"] == "numeric":
            parts.append(col.float().double().view(-1, 1) * W.view(1, -1))
            continue
        ids = col.long().view(col.shape[0], s["L"])
        e = F.embedding(ids, W, padding_idx=pad)                              # [B, L, D]
        keep = torch.ones(ids.shape, dtype=torch.float64)
        if s["pool"] in ("SUM_ID", "MEAN_ID") and s["mask_id"] is not None:
            keep = (ids != s["mask_id"]).double()
        eps = float(np.float32(s["eps"]))
        if s["pool"] == "NONE":
            parts.append(e[:, 0])
        elif s["pool"] == "CONCAT":
            parts.append(e.reshape(ids.shape[0], -1))
        elif s["pool"] in ("SUM", "SUM_ID"):
            parts.append((e * keep[:, :, None]).sum(1))
        elif s["pool"] == "MEAN_ID":
            parts.append((e * keep[:, :, None]).sum(1) / (keep.sum(1, keepdim=True) + eps))
        else:
            count = (e.detach().sum(2) != 0).double().sum(1, keepdim=True)
            parts.append(e.sum(1) / (count + eps))
    out = torch.cat(parts, 1)
    out.backward(dY.double())
    return out.detach(), {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}


@pytest.mark.parametrize("D,B", [(1, 5), (7, 33), (16, 64), (132, 9)])
def test_restatement_equals_float64_autograd_of_a_plain_composition(D, B):
    specs, tables, cols = grid_case(D, B, seed=D + B, big=40)
    specs.append(spec("dense", kind="dense"))
    cols["dense"] = torch.arange(B).double() / 3
    cols["one_3"] = cols["one_3"].double()                                    # a float id column
    _, width = widths(specs, tables)
    dY = torch.randn(B, width, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    lookups, t64 = lookups64(specs, tables, cols)
    out, a_out, c_out, grads = embed64(lookups, dY)
    want_out, want_grads = _composition(specs, tables, cols, dY)
    assert torch.allclose(out, want_out, rtol=1e-12, atol=1e-12)
    assert bool((a_out >= out.abs() - 1e-12).all())
    for key, t in t64.items():
        _, w, A = grads[id(t)]
        assert torch.allclose(w, want_grads[key].view(w.shape), rtol=1e-12, atol=1e-12), key
        assert bool((A >= w.abs() - 1e-12).all())
        assert bound_ratio(w.float(), w, A) <= 1.0                            # float32 rounding of the exact value passes
        pad = tables[key][1]
        if pad is not None:
            assert float(A[pad].abs().max()) == 0.0                           # the padding row: no gradient at all
    assert forward_ratio(out.float(), out, a_out, c_out) <= 1.0


# ---- 2. ... and means what the C oracle means ----------------------------------------------------------------------
_ORC_POOLS = ("NONE", "SUM", "MEAN_VALUE", "MEAN_ID", "SUM_ID", "CONCAT")


@pytest.mark.parametrize("B,D,id_dtype,Lh", [(1, 16, np.int64, 6), (77, 16, np.float64, 6), (300, 7, np.int32, 6),
                                             (129, 1, np.float32, 6), (64, 128, np.int64, 6), (33, 252, np.int64, 6),
                                             (40, 64, np.int64, 200), (9, 16, np.int32, 300), (20, 128, np.int64, 70),
                                             (12, 4, np.float64, 130), (7, 32, np.int64, 257), (5, 256, np.int64, 65)])
def test_restatement_against_the_c_oracle_within_its_sequential_rounding(B, D, id_dtype, Lh):
    """The shapes of test_embed_fwd_bwd_raw_cabi's _mixed_case through orc_embed_fwd / orc_embed_bwd (float32, sums left
    to right): every element within (n - 1) eps32 A of the restatement, n the number of terms it sums -- which pins the
    restatement's semantics (masks, padding rows, mean counts, shared tables) to the oracle the golden fixtures pin.
    Where a mean pool's scale (or a numeric feature's value) multiplied one of the terms the bound is n eps32 A: n - 1 additions, and the scale's own roundings
    (float32 reciprocal and product in the backward, the division in the forward: half an eps32 each), without which a
    row that ONE mean-pooled lookup reached would have to be exact -- the oracle's float32 product is not."""
    from oracle import c_oracle as C
    from test_gpu_cabi_vs_c_oracle import _mixed_case
    orc = C.load()
    block, W, specs, Lh = _mixed_case(B, D, seed=B + D, id_dtype=id_dtype, Lh=Lh)
    dW = {k: np.zeros_like(v) for k, v in W.items()}
    t64 = {k: Table(torch.from_numpy(v)) for k, v in W.items()}
    tblock = torch.from_numpy(block)
    host, lookups, off = [], [], 0
    for s in specs:
        one = (s["col"].stop - s["col"].start) == 1
        ids = block[:, s["col"].start] if one else block[:, s["col"]]
        kind = s.get("kind", C.CATEGORICAL)
        dim = 1 if kind == C.DENSE else D
        t = s["table"]
        f = C.field(ids, W[t] if t else None, dW[t] if t else None, kind=kind, dim=dim, out_off=off,
                    pool=s.get("pool", C.POOL_NONE), padding_idx=s.get("padding_idx"), mask_id=s.get("mask_id"),
                    eps=s.get("eps", 0.0))
        if kind == C.NUMERIC:
            f.vocab = 0
        host.append(f)
        col = tblock[:, s["col"].start] if one else tblock[:, s["col"]]
        lookups.append(Lookup64({C.CATEGORICAL: "categorical", C.NUMERIC: "numeric", C.DENSE: "dense"}[kind], col,
                                t64[t] if t else None, dim=dim, pool=_ORC_POOLS[s.get("pool", C.POOL_NONE)],
                                seq_len=1 if one else Lh, padding_idx=s.get("padding_idx"), mask_id=s.get("mask_id"),
                                eps=s.get("eps", 0.0), out_off=off))
        off += dim * (f.seq_len if f.pool == C.POOL_CONCAT else 1)
    n, width = len(host), off
    harr = C.array_of(host)
    out0 = np.zeros((B, width), np.float32)
    sc0 = np.zeros((n, B), np.float32)
    assert orc.orc_embed_fwd(harr, n, B, C.ptr(out0), width, C.ptr(sc0)) == 0
    R = np.random.default_rng(1).standard_normal((B, width)).astype(np.float32)
    orc.orc_embed_bwd(harr, n, B, C.ptr(R), width, C.ptr(sc0))
    counts = {}
    out, a_out, _, grads = embed64(lookups, torch.from_numpy(R), counts=counts)

    def worst(got, want, A, key):
        err = (torch.from_numpy(got).double().reshape(want.shape) - want).abs()
        terms = counts[key].reshape(want.shape) - 1 + (counts["scaled", key].reshape(want.shape) > 0).double()
        bound = terms.clamp(min=0) * EPS32 * A + 1e-30
        return float((err / bound).max())

    assert worst(out0, out, a_out, "out") <= 1.0
    for k, t in t64.items():
        _, want, A = grads[id(t)]
        assert worst(dW[k], want, A, id(t)) <= 1.0, k


# ---- 3. the bar is sharp ---------------------------------------------------------------------------------------------
def _one_table_case(ids, D, seed, V=1000, dY=None):
    gen = torch.Generator().manual_seed(seed)
    w = make_table(V, D, gen)
    B = ids.shape[0]
    L = ids.shape[1] if ids.dim() == 2 else 1
    if dY is None:
        dY = magnitudes((B, D), gen)
    table = Table(w)
    lk = Lookup64("categorical", ids, table, dim=D, pool="NONE" if L == 1 else "SUM_ID", seq_len=L, mask_id=-1 if L > 1 else None)
    out, a_out, c_out, grads = embed64([lk], dY)
    _, want, A = grads[id(table)]
    return w, dY.double(), out, a_out, c_out, want, A


def test_bound_rejects_one_lost_lookup_in_a_row_looked_up_once_and_in_a_row_of_2000():
    """|dY| >= 0.05, so one lost term is at least 0.05; a row of n lookups has A <= n and a bar of at most
    64 eps32 n = 7.6e-6 n: below 0.05 up to n of about 6 500."""
    gen = torch.Generator().manual_seed(3)
    ids = torch.randint(20, 1000, (6000,), generator=gen)
    ids[:2000] = 7
    ids[2000] = 9                                                            # looked up once
    ids = ids[torch.randperm(6000, generator=gen)]
    _, dY, _, _, _, want, A = _one_table_case(ids, 8, seed=4)
    for row, n in ((9, 1), (7, 2000)):
        assert int((ids == row).sum()) == n
        assert C_BOUND * EPS32 * n < 0.05 and float(A[row].max()) <= n        # the margin, by arithmetic
        got = want[row].float()                                              # a correct float32 evaluation
        assert bound_ratio(got, want[row], A[row]) <= 1.0
        b = int((ids == row).nonzero()[n // 2])
        assert bound_ratio(got.double() - dY[b], want[row], A[row]) > 1.0      # ... minus ONE lookup
        assert bound_ratio(got.double() - dY[b] + dY[b], want[row], A[row]) <= 1.0   # the bar, not the helper


def test_bound_rejects_a_lost_chunk_and_a_lost_window_in_the_hottest_row_of_the_hot_row_batch():
    """The GPU file's hot-row batch: id 7 collects ~70 000 of 100 000 lookups.  ONE term (about 0.5) is below that row's
    bar (64 eps32 A, about 0.27 at a mean magnitude of 0.5): the unit a fix-up can lose is a chunk's tail -- 16 consecutive
    sorted lookups -- and the hot id's samples carry a dY of one sign, so 16 terms sum to at least 0.8 > 64 eps32 70 000."""
    D = 4
    ids, sign = hot_row_batch(100000, seed=16)
    dY = hot_row_dy(sign, D, torch.Generator().manual_seed(17))
    _, dY, _, _, _, want, A = _one_table_case(ids.view(-1), D, seed=5, dY=dY)
    hot = (ids.view(-1) == 7).nonzero().view(-1)                             # sample order == sorted order (stable sort)
    n = hot.numel()
    assert 69000 < n < 71000
    bar = C_BOUND * EPS32 * float(A[7].max())
    assert float(A[7].max()) <= n and bar < 0.8 <= 16 * 0.05 + 1e-12          # the margin, by arithmetic
    got = want[7].float()
    assert bound_ratio(got, want[7], A[7]) <= 1.0
    for first, count in ((16 * 1234, 16), (16 * 512, 16 * 512)):              # one chunk; one window of 512 chunks
        lost = dY[hot[first:first + count]].sum(0)
        assert float(lost.min()) >= count * 0.05 - 1e-9
        assert bound_ratio(got.double() - lost, want[7], A[7]) > 1.0
        assert bound_ratio(got.double() - lost + lost, want[7], A[7]) <= 1.0


def test_forward_bound_rejects_one_lost_history_item_at_seq_len_300():
    """SUM over 300 rows with |w| in [0.05, 1]: A <= 300, C = 302, bar <= 302 eps32 300 = 0.011 < 0.05."""
    gen = torch.Generator().manual_seed(6)
    L = 300
    ids = torch.randint(0, 1000, (4, L), generator=gen)
    w, _, out, a_out, c_out, _, _ = _one_table_case(ids, 8, seed=7)
    assert float(c_out.max()) == L + 2 and (L + 2) * EPS32 * L < 0.05 and float(a_out.max()) <= L
    got = out.float()
    assert forward_ratio(got, out, a_out, c_out) <= 1.0
    lost = got.double().clone()
    lost[2] -= w[ids[2, 150]].double()
    assert forward_ratio(lost, out, a_out, c_out) > 1.0
    lost[2] += w[ids[2, 150]].double()
    assert forward_ratio(lost, out, a_out, c_out) <= 1.0


def test_copies_must_be_equal_and_untouched_rows_exactly_zero():
    ids = torch.tensor([1, 2, 2, 5])
    w, _, out, a_out, c_out, want, A = _one_table_case(ids, 4, seed=8, V=8)
    assert float(c_out.max()) == 0.0                                         # a one-id lookup is a copy
    got = out.float()
    assert forward_ratio(got, out, a_out, c_out) == 0.0
    got[1, 2] = torch.nextafter(got[1, 2], torch.tensor(2.0))
    assert forward_ratio(got, out, a_out, c_out) == float("inf")
    g = want.float()
    assert float(A[0].max()) == 0.0 and bound_ratio(g, want, A) <= 1.0
    g[0, 0] = 1e-20                                                          # a row nothing looked up
    assert bound_ratio(g, want, A) > 1.0
