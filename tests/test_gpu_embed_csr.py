"""The ragged (CSR) multi-hot lookup -- rbx_embed_csr_fwd / _sort / _bwd through ops.embed_bags -- against the float64
restatement of oracle/embed64.py, with the project's per-element bound |got - want| <= C eps32 A + tiny (backward:
C = C_BOUND; forward: max(C_BOUND, Lmax + 2)); elements with A = 0 must be exactly zero.

A ragged case is restated as a padded one: bag b becomes row b of a [B, L] id matrix whose tail holds the mask id
(SUM_ID / MEAN_ID) or the id of an all-zero table row (SUM / MEAN_VALUE).  To keep the float64 side affordable the samples
are restated in groups -- the few bags of several hundred ids at L = Lmax, the others at L = 40, in slices of the batch --
and the groups' outputs, gradients and absolute sums are merged into one ``Oracle`` (gradients are sums over samples).
The forward constant is max(C_BOUND, Lmax + 2) on every row.

Forms: bag_walk_kernel<PoolOp, SG, R, NV, VEC> takes the instantiation embed_seq_kernel takes for the dim (the table in
tests/test_gpu_embed_dims.py), and sums a bag in that kernel's order: the outputs of the id-masked pools are bit-equal
to the padded call's at every dim and every bag length (there is no separate long-bag form; none is exempt)."""
import pytest
import torch

from conftest import _note
from oracle.embed64 import C_BOUND, bound_ratio
from test_embed64_restatement import hot_row_batch, hot_row_dy, magnitudes, make_table, spec
from test_gpu_embed_dims import COMPACT_ABOVE, SCALAR_NV1, SCALAR_NVN, VEC_NV1, VEC_NVN, Device, Oracle, form

pytestmark = pytest.mark.gpu

_POOL = {"SUM": 1, "MEAN_VALUE": 2, "MEAN_ID": 3, "SUM_ID": 4}
SHORT = 40                       # most bags have 0 .. SHORT ids
SLICE_ELEMS = 24 << 20           # float64 elements of one restated [samples, L, D] block at most


# ---- ragged cases and their padded restatement --------------------------------------------------------------------------
class Ragged(object):
    """One feature's bags on the CPU: ``ids`` (list of 1-D int64 tensors), its pool, table key, mask id and eps."""

    def __init__(self, name, table, pool, ids, mask_id=None, eps=0.0, fill=0):
        self.name, self.table, self.pool, self.ids, self.mask_id, self.eps, self.fill = name, table, pool, ids, mask_id, eps, fill
        self.lengths = torch.tensor([t.numel() for t in ids], dtype=torch.int64)

    def padded(self, L, samples=None):
        pick = range(len(self.ids)) if samples is None else samples.tolist()
        out = torch.full((len(pick), L), self.fill, dtype=torch.int64)
        for r, b in enumerate(pick):
            out[r, :self.ids[b].numel()] = self.ids[b]
        return out

    def spec(self, L):
        return spec(self.name, table=self.table, pool=self.pool, L=L, mask_id=self.mask_id, eps=self.eps)

    def bags(self, idx_dtype=torch.int64, off_dtype=torch.int64, junk=(0, 0), junk_id=0):
        """ops.Bags on the GPU; ``junk`` = ids in front of the first and behind the last bag that belong to no bag."""
        from recbox_amd import ops
        flat = torch.cat([torch.full((junk[0],), junk_id, dtype=torch.int64)] + list(self.ids)
                         + [torch.full((junk[1],), junk_id, dtype=torch.int64)])
        offsets = torch.zeros(len(self.ids) + 1, dtype=torch.int64)
        torch.cumsum(self.lengths, 0, out=offsets[1:])
        return ops.Bags(flat.to(idx_dtype).cuda(), (offsets + junk[0]).to(off_dtype).cuda())


def _bag_ids(V, lengths, gen, lo=1, masked_frac=0.0):
    out = []
    for n in lengths.tolist():
        ids = torch.randint(lo, V, (n,), generator=gen)
        if masked_frac:
            ids[torch.rand(n, generator=gen) < masked_frac] = 0
        out.append(ids)
    return out


def _lengths(B, gen, n_long):
    lengths = torch.randint(0, SHORT + 1, (B,), generator=gen)
    where = torch.randperm(B, generator=gen)[:n_long]
    lengths[where] = torch.randint(300, 700, (where.numel(),), generator=gen)
    return lengths


def grid_bags(D, B, seed, big):
    """Four features, one per pool: SUM and MEAN_VALUE share the 300-row table (rows 5 and 17 all zeros and not the padding
    row; row 0, the padding row, is the all-zero fill of the restatement), SUM_ID over 3 rows (each row collects thousands
    of lookups: the long fix-up), MEAN_ID over ``big`` rows; ~10 % of the id pools' ids are the mask id inside the bags."""
    gen = torch.Generator().manual_seed(seed)
    tables = {"T3": (make_table(3, D, gen, pad=0), 0),
              "T300": (make_table(300, D, gen, pad=0, zero_rows=(5, 17), value_mask_safe=True), 0),
              "Tbig": (make_table(big, D, gen, pad=0), 0)}
    n_long = min(B, 5)
    feats = [Ragged("sum", "T300", "SUM", _bag_ids(300, _lengths(B, gen, n_long), gen)),
             Ragged("mean_value", "T300", "MEAN_VALUE", _bag_ids(300, _lengths(B, gen, n_long), gen), eps=1e-12),
             Ragged("sum_id", "T3", "SUM_ID", _bag_ids(3, _lengths(B, gen, n_long), gen, masked_frac=0.1), mask_id=0),
             Ragged("mean_id", "Tbig", "MEAN_ID", _bag_ids(big, _lengths(B, gen, n_long), gen, masked_frac=0.1), mask_id=0,
                    eps=1e-16)]
    return feats, tables


def merged_oracle(feats, tables, dY):
    """``Oracle`` of the whole ragged case, merged from restatements of sample groups (see the module docstring)."""
    B = dY.shape[0]
    D = max(w.shape[-1] for w, _ in tables.values())
    longest = torch.stack([f.lengths for f in feats]).max(0).values
    Lmax = max(int(longest.max()), 1)
    groups = []
    long_ones = (longest > SHORT).nonzero().view(-1)
    if long_ones.numel():
        groups.append((long_ones, Lmax))
    short_ones = (longest <= SHORT).nonzero().view(-1)
    per = max(1, SLICE_ELEMS // (SHORT * D))
    for i in range(0, short_ones.numel(), per):
        groups.append((short_ones[i:i + per], max(min(SHORT, Lmax), 1)))
    runs = []
    for samples, L in groups:
        cols = {f.name: f.padded(L, samples) for f in feats}
        runs.append((samples, Oracle([f.spec(L) for f in feats], tables, cols, dY[samples])))
    top = Oracle.__new__(Oracle)
    width = runs[0][1].out.shape[1]
    top.out = torch.zeros(B, width, dtype=torch.float64)
    top.a_out = torch.zeros(B, width, dtype=torch.float64)
    top.c_out = torch.full((width,), float(max(C_BOUND, Lmax + 2)), dtype=torch.float64)
    for samples, o in runs:
        top.out[samples], top.a_out[samples] = o.out, o.a_out
    top.t64, top.rows, top.grads = runs[0][1].t64, {}, {}
    for key, t in top.t64.items():
        parts = [(o.rows.get(key), o.grads.get(id(o.t64[key]))) for _, o in runs]
        parts = [(rows, ent) for rows, ent in parts if ent is not None]
        if not parts:
            continue
        if tables[key][0].shape[0] > COMPACT_ABOVE:
            union = torch.unique(torch.cat([rows for rows, _ in parts]))
            top.rows[key] = union
            want = torch.zeros(union.numel(), parts[0][1][1].shape[1], dtype=torch.float64)
            A = torch.zeros_like(want)
            for rows, (_, w, a) in parts:
                at = torch.searchsorted(union, rows)
                want[at] += w
                A[at] += a
        else:
            want = sum(w for _, (_, w, a) in parts)
            A = sum(a for _, (_, w, a) in parts)
        top.grads[id(t)] = (t, want, A)
    return top, Lmax


class BagDevice(object):
    """The tables as nn.Embedding modules on the GPU (shared with a padded ``Device`` when given) and the BagPlan."""

    def __init__(self, feats, tables, modules=None):
        from recbox_amd import ops
        self.feats, self.modules = feats, dict(modules or {})
        for key, (w, pad) in tables.items():
            if key not in self.modules:
                m = torch.nn.Embedding(w.shape[0], w.shape[1], padding_idx=pad)
                m.weight.data.copy_(w)
                self.modules[key] = m.cuda()
        self.keys = []
        specs, off = [], 0
        for f in feats:
            if f.table not in self.keys:
                self.keys.append(f.table)
            m = self.modules[f.table]
            specs.append(ops.BagSpec(f.name, m.embedding_dim, off, self.keys.index(f.table), _POOL[f.pool], m.num_embeddings,
                                     padding_idx=m.padding_idx, mask_id=f.mask_id, eps=f.eps))
            off += m.embedding_dim
        self.plan, self.width = ops.BagPlan(specs), off

    def params(self):
        return [self.modules[k].weight for k in self.keys]

    def zero_grad(self):
        for m in self.modules.values():
            m.weight.grad = None

    def step(self, bags, dY, retain_graph=False):
        from recbox_amd import ops
        out = ops.embed_bags(self.plan, bags, self.params())
        out.backward(dY.cuda(), retain_graph=retain_graph)
        torch.cuda.synchronize()
        return out

    def grads(self):
        return {k: (m.weight.grad if m.weight.grad is not None else torch.zeros_like(m.weight)) for k, m in self.modules.items()}


def _dy(B, width, seed):
    return magnitudes((B, width), torch.Generator().manual_seed(seed))


# ---- the dim grid ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", VEC_NV1 + VEC_NVN + SCALAR_NV1 + SCALAR_NVN)
def test_bags_grid_of_dims_against_float64_and_the_padded_path(D):
    """Four bags per call (one per pool, two sharing a table), tables of 3, 300 and 200 000 rows (fewer beyond D = 256),
    bag lengths 0 .. 40 plus five of 300 .. 699 per feature, B = 6181 and B = 1; int64 indices with int32 offsets and ids in
    front of offsets[0] / behind offsets[B] that are OUT OF RANGE (nothing may read them), float64 indices with int64
    offsets.  Then the padded call over the same ids at L = Lmax: its id-masked pools' outputs are bit-equal to the bags',
    and its gradients meet the same float64 bound."""
    big = 200000 if D <= 256 else 200000 * 256 // D
    for B in (6181, 1):
        feats, tables = grid_bags(D, B, seed=1000 * D + B, big=big)
        dY = _dy(B, 4 * D, seed=D + B)
        oracle, Lmax = merged_oracle(feats, tables, dY)
        dev = BagDevice(feats, tables)
        outs = []
        for tag, kw in (("i64/i32 junk", dict(idx_dtype=torch.int64, off_dtype=torch.int32, junk=(5, 9), junk_id=1 << 40)),
                        ("f64/i64", dict(idx_dtype=torch.float64, off_dtype=torch.int64))):
            dev.zero_grad()
            out = dev.step([f.bags(**kw) for f in feats], dY)
            oracle.check("bags D%d B%d %s" % (D, B, tag), form(D) + " bags", out.detach(), dev.grads())
            pad_grad = dev.grads()["T300"][0]
            assert int(torch.count_nonzero(pad_grad)) == 0                  # the padding_idx row
            outs.append(out.detach())
        assert torch.equal(outs[0], outs[1])
        padded = Device([f.spec(Lmax) for f in feats], tables, modules=dev.modules)
        dev.zero_grad()
        out_p = padded.step({f.name: f.padded(Lmax) for f in feats}, dY)
        oracle.check("padded D%d B%d" % (D, B), form(D) + " bags' padded twin", out_p.detach(), padded.grads())
        for k, f in enumerate(feats):
            if f.pool in ("SUM_ID", "MEAN_ID"):
                assert torch.equal(out_p.detach()[:, k * D:(k + 1) * D], outs[0][:, k * D:(k + 1) * D]), \
                    "D%d B%d %s: bags and padded outputs differ" % (D, B, f.name)


@pytest.mark.parametrize("D", [257, 1028])
def test_bag_dims_without_a_lane_group_form_are_refused_and_nothing_is_written(D):
    from recbox_amd import _lib, ops
    gen = torch.Generator().manual_seed(D)
    w = torch.nn.Parameter(make_table(50, D, gen).cuda())
    bags = ops.Bags(torch.randint(0, 50, (40,), generator=gen).cuda(), torch.tensor([0, 7, 40]).cuda())
    plan = ops.BagPlan([ops.BagSpec("h", D, 0, 0, _POOL["SUM"], 50)])
    with pytest.raises(NotImplementedError):
        ops.embed_bags(plan, [bags], [w])
    plan.bind_inputs([bags])
    plan.bind_params([w], [w])
    out = torch.zeros(2, D, device="cuda")
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    assert _lib.lib.rbx_embed_csr_fwd(plan.arr, 1, 2, out.data_ptr(), D, None, None, None) == _lib.RBX_ERR_UNSUPPORTED
    assert _lib.lib.rbx_embed_csr_bwd_workspace_size(plan.arr, 1, 2) == 0
    assert _lib.lib.rbx_embed_csr_sort(plan.arr, 1, 2, ws.data_ptr(), ws.numel(), None, None) == _lib.RBX_ERR_UNSUPPORTED
    assert _lib.lib.rbx_embed_csr_bwd(plan.arr, 1, 2, out.data_ptr(), D, None, 0, ws.data_ptr(), ws.numel(),
                                      None) == _lib.RBX_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert int(torch.count_nonzero(out)) == 0 and int(torch.count_nonzero(ws)) == 0
    w4 = torch.nn.Parameter(make_table(50, 4, gen).cuda())                  # ... and the next call runs
    out = ops.embed_bags([ops.BagSpec("h", 4, 0, 0, _POOL["SUM"], 50)], [bags], [w4])
    want = torch.stack([w4.detach()[bags.indices[:7]].double().sum(0), w4.detach()[bags.indices[7:]].double().sum(0)])
    assert float((out.detach().double() - want).abs().max()) < 1e-4


# ---- backward: hot rows, repeatability ------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [16, 132, 256])
def test_hot_rows_in_bags_against_float64_and_two_backwards_over_one_sort(D):
    """~100 000 lookups in bags of 1 .. 7 ids, 70 % of them on row 7 and 20 % on row 3 (chains that the long fix-up splits
    over workgroups), non-zero dY everywhere.  Two backwards over the one sort of the forward are bit-identical."""
    ids, sign = hot_row_batch(100000, seed=16, L=7)
    gen = torch.Generator().manual_seed(D + 5)
    B = ids.shape[0]
    lengths = torch.randint(1, 8, (B,), generator=gen)
    lengths[(ids == 7).any(1)] = 7                                          # (the sign recipe is per sample: keep row 7's samples whole)
    feat = Ragged("hot", "T", "SUM_ID", [ids[b, :int(n)] for b, n in enumerate(lengths.tolist())], mask_id=0)
    tables = {"T": (make_table(1000, D, gen), None)}
    dY = hot_row_dy(sign, D, gen)
    oracle = Oracle([feat.spec(7)], tables, {"hot": feat.padded(7)}, dY)
    dev = BagDevice([feat], tables)
    out = dev.step([feat.bags()], dY, retain_graph=True)
    oracle.check("hot rows in bags D%d" % D, form(D) + " bags hot rows", out.detach(), dev.grads())
    first = dev.grads()["T"].clone()
    dev.zero_grad()
    out.backward(dY.cuda())
    torch.cuda.synchronize()
    assert torch.equal(dev.grads()["T"], first)


# ---- edges ----------------------------------------------------------------------------------------------------------------
def _one_feature(pool="MEAN_ID", D=16, V=300, seed=3, **kw):
    gen = torch.Generator().manual_seed(seed)
    tables = {"T": (make_table(V, D, gen, pad=0), 0)}
    return gen, tables, dict(mask_id=0 if pool.endswith("_ID") else None, eps=1e-8 if pool.startswith("MEAN") else 0.0, **kw)


@pytest.mark.parametrize("pool", ["SUM", "MEAN_ID"])
def test_all_bags_empty(pool):
    gen, tables, kw = _one_feature(pool)
    B = 77
    feat = Ragged("h", "T", pool, [torch.zeros(0, dtype=torch.int64)] * B, **kw)
    dev = BagDevice([feat], tables)
    for junk in ((0, 0), (3, 4)):                                           # nnz == 0, and ids that no bag owns
        dev.zero_grad()
        out = dev.step([feat.bags(junk=junk, junk_id=5)], _dy(B, 16, 1))
        assert int(torch.count_nonzero(out)) == 0 and not bool(torch.isnan(out).any())
        assert int(torch.count_nonzero(dev.grads()["T"])) == 0


def test_every_id_masked():
    gen, tables, kw = _one_feature("MEAN_ID")
    B = 257
    lengths = torch.randint(0, 30, (B,), generator=gen)
    feats = [Ragged("m", "T", "MEAN_ID", [torch.zeros(int(n), dtype=torch.int64) for n in lengths], **kw),
             Ragged("s", "T", "SUM_ID", [torch.zeros(int(n), dtype=torch.int64) for n in lengths], mask_id=0)]
    dev = BagDevice(feats, tables)
    out = dev.step([f.bags() for f in feats], _dy(B, 32, 1))
    assert int(torch.count_nonzero(out)) == 0
    assert int(torch.count_nonzero(dev.grads()["T"])) == 0


def test_batch_of_zero_bags():
    from recbox_amd import ops
    gen, tables, kw = _one_feature("SUM")
    dev = BagDevice([Ragged("h", "T", "SUM", [], **kw)], tables)
    bags = ops.Bags(torch.tensor([4, 5, 6]).cuda(), torch.tensor([1]).cuda())
    out = ops.embed_bags(dev.plan, [bags], dev.params())
    assert tuple(out.shape) == (0, 16)
    out.sum().backward()
    torch.cuda.synchronize()
    assert int(torch.count_nonzero(dev.grads()["T"])) == 0


@pytest.mark.parametrize("D", [16, 132])
def test_one_bag_holds_every_id(D):
    gen, tables, kw = _one_feature("MEAN_ID", D=D)
    n = 5000
    ids = torch.randint(0, 300, (n,), generator=gen)
    feats = [Ragged("m", "T", "MEAN_ID", [ids], **kw), Ragged("s", "T", "SUM", [ids.clone()])]
    dY = _dy(1, 2 * D, 2)
    oracle = Oracle([f.spec(n) for f in feats], tables, {f.name: f.padded(n) for f in feats}, dY)
    dev = BagDevice(feats, tables)
    out = dev.step([f.bags() for f in feats], dY)
    oracle.check("one bag of %d ids D%d" % (n, D), form(D) + " one bag", out.detach(), dev.grads())


def test_malformed_offsets_raise_and_leave_the_well_formed_bags_correct():
    """A decreasing pair, and offsets[B] = nnz + 7.  ``indices`` is a view into the middle of a larger buffer of valid ids,
    so even a kernel that did not clamp would read mapped memory.  With config.check_ids the call raises IndexError (the
    class an out-of-range id raises); with the deferred check it runs, check_deferred_ids() raises, and every bag whose
    own pair of offsets is intact -- the whole well-formed feature and the untouched bags of the malformed ones -- equals
    the clean call's."""
    from recbox_amd import ops
    gen, tables, kw = _one_feature("MEAN_ID")
    B = 200
    lengths = torch.randint(0, 12, (B,), generator=gen)
    lengths[10:14] = torch.tensor([6, 5, 7, 4])
    ids = _bag_ids(300, lengths, gen)
    feats = [Ragged(n, "T", "MEAN_ID", ids, **kw) for n in ("good", "decreasing", "beyond")]
    dev = BagDevice(feats, tables)
    nnz = int(lengths.sum())
    buf = torch.full((nnz + 4000,), 7, dtype=torch.int64, device="cuda")
    flat = buf[2000:2000 + nnz]
    flat.copy_(torch.cat(ids))
    offsets = torch.zeros(B + 1, dtype=torch.int64)
    torch.cumsum(lengths, 0, out=offsets[1:])
    dec = offsets.clone()
    dec[12] = dec[11] - 3                                                   # bag 11 = [o11, o11 - 3): decreasing; bag 12 starts early
    bey = offsets.clone()
    bey[B] = nnz + 7
    clean = [ops.Bags(flat, offsets.cuda())] * 3
    bad = [ops.Bags(flat, offsets.cuda()), ops.Bags(flat, dec.cuda()), ops.Bags(flat, bey.cuda())]
    with torch.no_grad():
        want = ops.embed_bags(dev.plan, clean, dev.params())
    old = ops.config.check_ids
    try:
        with pytest.raises(IndexError):
            ops.embed_bags(dev.plan, bad, dev.params())                      # training mode: the sort clamps the same way
        ops.config.check_ids = False
        try:
            ops.check_deferred_ids()                                         # (reads and clears what earlier calls left)
        except IndexError:
            pass
        out = ops.embed_bags(dev.plan, bad, dev.params())
        with pytest.raises(IndexError):
            ops.check_deferred_ids()
        with torch.no_grad():
            ops.embed_bags(dev.plan, clean, dev.params())
        ops.check_deferred_ids()                                             # a clean call raises nothing
    finally:
        ops.config.check_ids = old
    torch.cuda.synchronize()
    out, D = out.detach(), 16
    assert torch.equal(out[:, :D], want[:, :D])
    intact = torch.ones(B, dtype=torch.bool)
    intact[11:13] = False
    assert torch.equal(out[intact, D:2 * D], want[intact, D:2 * D])
    assert int(torch.count_nonzero(out[11, D:2 * D])) == 0                   # the decreasing pair: an empty bag
    assert torch.equal(out[:B - 1, 2 * D:], want[:B - 1, 2 * D:])


# ---- one captured step ----------------------------------------------------------------------------------------------------
def test_forward_and_backward_captured_in_one_graph_replay_on_new_contents():
    """Forward + backward of ops.embed_bags in one torch.cuda.graph on one stream; ``indices`` / ``offsets`` overwritten in
    place (same nnz, other bag boundaries), replayed: outputs and gradients equal an eager run on the new contents."""
    from recbox_amd import ops
    gen, tables, kw = _one_feature("MEAN_ID", D=32, V=5000)
    B, nnz = 513, 9000

    def contents(seed):
        g = torch.Generator().manual_seed(seed)
        cuts = torch.sort(torch.randint(0, nnz + 1, (B - 1,), generator=g)).values
        offsets = torch.cat([torch.zeros(1, dtype=torch.int64), cuts, torch.tensor([nnz])])
        return torch.randint(0, 5000, (nnz,), generator=g), offsets

    feats = [Ragged("m", "T", "MEAN_ID", [], **kw), Ragged("s", "T", "SUM", [])]
    dev = BagDevice(feats, tables)
    idx0, off0 = contents(1)
    indices, offsets = idx0.cuda(), off0.to(torch.int32).cuda()
    bags = [ops.Bags(indices, offsets)] * 2
    dY = _dy(B, 64, 3).cuda()
    w = dev.modules["T"].weight
    old = ops.config.check_ids
    try:
        ops.config.check_ids = False
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                w.grad = None
                ops.embed_bags(dev.plan, bags, dev.params()).backward(dY)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        w.grad = None
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = ops.embed_bags(dev.plan, bags, dev.params())
            out.backward(dY)
        grad = w.grad
        idx1, off1 = contents(2)
        indices.copy_(idx1.cuda())
        offsets.copy_(off1.to(torch.int32).cuda())
        graph.replay()
        torch.cuda.synchronize()
        got_out, got_grad = out.detach().clone(), grad.clone()
        w.grad = None
        want_out = ops.embed_bags(dev.plan, [ops.Bags(idx1.cuda(), off1.cuda())] * 2, dev.params())
        want_out.backward(dY)
        torch.cuda.synchronize()
        ops.check_deferred_ids()
    finally:
        ops.config.check_ids = old
    assert torch.equal(got_out, want_out.detach())
    assert torch.equal(got_grad, w.grad)
    assert int(torch.count_nonzero(got_grad)) > 0


# ---- the rechub layer -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("squeeze_dim", [True, False])
def test_rechub_embedding_layer_takes_bags_for_pooled_sequence_features(squeeze_dim):
    """Two sparse and two sequence features (one shared_with a sparse one): fed padded and fed as ops.Bags the layer gives
    bit-equal outputs; both runs' gradients meet the float64 bound (the shared table gets ONE gradient from the bag node
    and the padded node of the pass).  pooling='concat' with Bags raises ValueError."""
    from recbox_amd import ops
    from recbox_amd.rechub.basic.features import SequenceFeature, SparseFeature
    from recbox_amd.rechub.basic.layers import EmbeddingLayer
    gen = torch.Generator().manual_seed(11)
    B, L, D = 1500, 20, 16
    feats = [SparseFeature("a", 50, D), SparseFeature("b", 300, D),
             SequenceFeature("hist_b", 300, D, pooling="mean", shared_with="b", padding_idx=0),
             SequenceFeature("hist_c", 700, D, pooling="sum", padding_idx=0)]
    layer = EmbeddingLayer(feats).cuda()
    tables = {}
    for key in ("a", "b", "hist_c"):
        w = make_table(layer.embed_dict[key].num_embeddings, D, gen)
        layer.embed_dict[key].weight.data.copy_(w)
        tables[key] = (w, layer.embed_dict[key].padding_idx)
    from test_embed64_restatement import history
    cols = {"a": torch.randint(0, 50, (B,), generator=gen), "b": torch.randint(0, 300, (B,), generator=gen),
            "hist_b": history(300, B, L, gen, empty_frac=0.05), "hist_c": history(700, B, L, gen)}
    specs = [spec("a", table="a"), spec("b", table="b"), spec("hist_b", table="b", pool="MEAN_ID", L=L, mask_id=0, eps=1e-16),
             spec("hist_c", table="hist_c", pool="SUM_ID", L=L, mask_id=0)]
    dY = _dy(B, 4 * D, 5)
    oracle = Oracle(specs, tables, cols, dY)
    x_pad = {k: v.cuda() for k, v in cols.items()}
    x_bag = dict(x_pad, hist_b=ops.bags_from_padded(x_pad["hist_b"], 0), hist_c=ops.bags_from_padded(x_pad["hist_c"], 0))
    outs = []
    for tag, x in (("padded", x_pad), ("bags", x_bag)):
        for m in layer.embed_dict.values():
            m.weight.grad = None
        out = layer(x, feats, squeeze_dim=squeeze_dim)
        assert tuple(out.shape) == ((B, 4 * D) if squeeze_dim else (B, 4, D))
        out.backward(dY.cuda().view(out.shape))
        torch.cuda.synchronize()
        grads = {k: layer.embed_dict[k].weight.grad for k in tables}
        oracle.check("rechub layer %s squeeze=%s" % (tag, squeeze_dim), form(D) + " layer " + tag, out.detach().reshape(B, -1), grads)
        outs.append(out.detach().reshape(B, -1).clone())
    assert torch.equal(outs[0], outs[1])
    concat = [SequenceFeature("hist_k", 300, D, pooling="concat", padding_idx=0)]
    layer_k = EmbeddingLayer(concat).cuda()
    with pytest.raises(ValueError):
        layer_k({"hist_k": x_bag["hist_b"]}, concat, squeeze_dim=squeeze_dim)
