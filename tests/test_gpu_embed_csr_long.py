"""The long-bag form of the ragged (CSR) lookup -- rbx_embed_csr_fwd_long / _fwd_weighted_long / _weight_grad_long, through
ops.embed_bags with ops.bag_long_threshold(64) and through _lib -- at bag lengths on every side of the threshold (64) and of
the segment size (256): 0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1300.

Bounds are those of tests/test_gpu_embed_csr.py and tests/test_gpu_embed_csr_weighted.py: |got - want| <= C eps32 A + tiny
against float64, forward C = max(C_BOUND, Lmax + 2) (a long bag is summed per segment and then over its segments: any
order of float32 additions of L terms meets the L + 2 constant), gradients C = C_BOUND, weight gradient
C = max(C_BOUND, D + 2).  Bags below the threshold are bit-equal to the lane-group calls; bags at or above it are
bit-identical from run to run.

The float64 side is ``merged_oracle``'s merge over sample groups with one change: the groups are the length classes
(<= 65, <= 257, <= 513, 1300 ids), each restated at its own L, instead of "everything above 40 ids at Lmax" -- the same
sums at a quarter of the padded elements.  All four features of a case share one permutation of the lengths for that."""
import pytest
import torch

from oracle.embed64 import C_BOUND, bound_ratio
from test_embed64_restatement import magnitudes, make_table
from test_gpu_embed_csr import BagDevice, Ragged, _bag_ids
from test_gpu_embed_csr_weighted import SUM, SUM_ID, Dev, Feature, _weights, check
from test_gpu_embed_dims import COMPACT_ABOVE, SCALAR_NV1, SCALAR_NVN, VEC_NV1, VEC_NVN, Oracle, form

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1300]
CLASSES = [65, 257, 513, 1300]
T, S, B0 = 64, 256, 97


@pytest.fixture(autouse=True)
def threshold_64():
    from recbox_amd import ops
    old = ops.bag_long_threshold(T)
    try:
        yield
    finally:
        ops.bag_long_threshold(old)


def _dy(B, width, seed):
    return magnitudes((B, width), torch.Generator().manual_seed(seed))


def edge_lengths(B, gen):
    if B == 1:
        return torch.tensor([1300])
    reps = (LENGTHS * (B // len(LENGTHS) + 1))[:B]
    return torch.tensor(reps)[torch.randperm(B, generator=gen)]


def edge_bags(D, B, seed):
    """grid_bags' four features (SUM and MEAN_VALUE on the 300-row table with two zero rows, SUM_ID on 3 rows, MEAN_ID on
    5 000 rows; ~10 % masked ids in the id pools) at LENGTHS, repeated and shuffled over the batch."""
    gen = torch.Generator().manual_seed(seed)
    tables = {"T3": (make_table(3, D, gen, pad=0), 0),
              "T300": (make_table(300, D, gen, pad=0, zero_rows=(5, 17), value_mask_safe=True), 0),
              "Tbig": (make_table(5000, D, gen, pad=0), 0)}
    lengths = edge_lengths(B, gen)
    feats = [Ragged("sum", "T300", "SUM", _bag_ids(300, lengths, gen)),
             Ragged("mean_value", "T300", "MEAN_VALUE", _bag_ids(300, lengths, gen), eps=1e-12),
             Ragged("sum_id", "T3", "SUM_ID", _bag_ids(3, lengths, gen, masked_frac=0.1), mask_id=0),
             Ragged("mean_id", "Tbig", "MEAN_ID", _bag_ids(5000, lengths, gen, masked_frac=0.1), mask_id=0, eps=1e-16)]
    return feats, tables


def class_oracle(feats, tables, dY):
    """``merged_oracle`` (tests/test_gpu_embed_csr.py) with the length classes as its sample groups."""
    B = dY.shape[0]
    longest = torch.stack([f.lengths for f in feats]).max(0).values
    Lmax = max(int(longest.max()), 1)
    runs, lo = [], -1
    for L in CLASSES:
        samples = ((longest > lo) & (longest <= L)).nonzero().view(-1)
        lo = L
        if samples.numel():
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
    return top


def expected_counts(lengths_per_feature, threshold=T):
    """(bags that take the long form, their segments) from the CPU's lengths."""
    n_long = n_seg = 0
    for lengths in lengths_per_feature:
        long_ones = lengths[lengths >= threshold]
        n_long += int(long_ones.numel())
        n_seg += int(((long_ones + S - 1) // S).sum())
    return n_long, n_seg


def header(ws):
    from recbox_amd import _lib
    words = ws[:8].view(torch.int32).tolist()
    return words[_lib.CSR_WS_LONG_BAGS], words[_lib.CSR_WS_SEGMENTS]


# ---- 1. lengths at every edge, every lane-group form ---------------------------------------------------------------------
@pytest.mark.parametrize("D", VEC_NV1 + VEC_NVN + SCALAR_NV1 + SCALAR_NVN)
def test_long_bags_at_every_length_edge_against_float64(D):
    for B in (B0, 1):
        feats, tables = edge_bags(D, B, seed=1000 * D + B)
        dY = _dy(B, 4 * D, seed=D + B)
        oracle = class_oracle(feats, tables, dY)
        dev = BagDevice(feats, tables)
        out = dev.step([f.bags(idx_dtype=torch.int64, off_dtype=torch.int32, junk=(5, 9), junk_id=1 << 40) for f in feats], dY)
        assert header(dev.plan._long_ws) == expected_counts([f.lengths for f in feats])     # the long form did run
        oracle.check("long bags D%d B%d" % (D, B), form(D) + " long bags", out.detach(), dev.grads())
        assert int(torch.count_nonzero(dev.grads()["T300"][0])) == 0                        # the padding_idx row


# ---- 2. / 3. the dispatch is what it claims, and repeats itself -----------------------------------------------------------
class Direct(object):
    """The four features at D = 16 bound to a BagPlan, and the C calls on buffers of the test's own."""

    def __init__(self, B=B0, seed=5):
        from recbox_amd import _lib
        self.D = 16
        self.feats, tables = edge_bags(self.D, B, seed)
        self.dev = BagDevice(self.feats, tables)
        self.bags = [f.bags() for f in self.feats]
        self.B, self.n, self.width = B, len(self.feats), 4 * self.D
        self.dev.plan.bind_inputs(self.bags)
        self.dev.plan.bind_params(self.dev.params())
        self.lib, self.arr = _lib.lib, self.dev.plan.arr

    def ws(self, threshold):
        need = self.lib.rbx_embed_csr_fwd_long_workspace_size(self.arr, self.n, self.B, threshold)
        assert need >= 256
        return torch.full((need,), 0x5A, dtype=torch.uint8, device="cuda"), need

    def fwd_long(self, threshold):
        from recbox_amd import _lib, ops
        out = torch.full((self.B, self.width), 7.0, device="cuda")
        scale = torch.full((self.n, self.B), 7.0, device="cuda")
        ws, need = self.ws(threshold)
        _lib.check(self.lib.rbx_embed_csr_fwd_long(self.arr, self.n, self.B, threshold, out.data_ptr(), self.width, scale.data_ptr(),
                                                   ws.data_ptr(), need, None, ops._stream()))
        torch.cuda.synchronize()
        return out, scale, ws

    def fwd(self):
        from recbox_amd import _lib, ops
        out = torch.full((self.B, self.width), 7.0, device="cuda")
        scale = torch.full((self.n, self.B), 7.0, device="cuda")
        _lib.check(self.lib.rbx_embed_csr_fwd(self.arr, self.n, self.B, out.data_ptr(), self.width, scale.data_ptr(), None,
                                              ops._stream()))
        torch.cuda.synchronize()
        return out, scale


def test_header_counts_threshold_zero_and_short_bags_bit_equal_to_the_lane_group_call():
    from recbox_amd import _lib
    d = Direct()
    out_l, scale_l, ws = d.fwd_long(T)
    assert header(ws) == expected_counts([f.lengths for f in d.feats])
    assert header(ws)[0] > 0
    out_p, scale_p = d.fwd()
    out_0, scale_0, ws_0 = d.fwd_long(0)
    assert header(ws_0) == (0, 0)
    assert torch.equal(out_0, out_p) and torch.equal(scale_0, scale_p)
    for k, f in enumerate(d.feats):                                         # short bags: the same bits beside long ones
        short = (f.lengths < T).cuda()
        assert int(short.sum()) > 0 and int((~short).sum()) > 0
        assert torch.equal(out_l[short, k * d.D:(k + 1) * d.D], out_p[short, k * d.D:(k + 1) * d.D])
        if f.pool.startswith("MEAN"):
            assert torch.equal(scale_l[k][short], scale_p[k][short])
            assert bool((scale_l[k] != 7.0).all())                          # every bag's scale is written, long ones included
    small = d.ws(T)[1] - 256                                                # a workspace that is too small is refused
    buf = torch.zeros(max(small, 1), dtype=torch.uint8, device="cuda")
    out = torch.zeros(d.B, d.width, device="cuda")
    assert d.lib.rbx_embed_csr_fwd_long(d.arr, d.n, d.B, T, out.data_ptr(), d.width, scale_p.data_ptr(), buf.data_ptr(), small,
                                        None, None) == _lib.RBX_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert int(torch.count_nonzero(out)) == 0 and int(torch.count_nonzero(buf)) == 0


def test_two_long_calls_give_the_same_bits():
    d = Direct(seed=6)
    first, scale_1, _ = d.fwd_long(T)
    second, scale_2, _ = d.fwd_long(T)
    assert torch.equal(first, second) and torch.equal(scale_1, scale_2)
    assert not bool(torch.isnan(first).any())


# ---- 4. weighted ----------------------------------------------------------------------------------------------------------
def _weighted_case(D, B, seed, ones=False):
    ragged, tables = edge_bags(D, B, seed)
    gen = torch.Generator().manual_seed(seed + 1)
    feats = []
    for r in ragged:
        if r.pool in ("SUM", "SUM_ID"):
            n = int(r.lengths.sum())
            w = torch.ones(n) if ones else _weights(n, gen, 0.05)
            feats.append(Feature(r.name, r.table, SUM if r.pool == "SUM" else SUM_ID, r.ids, w, r.mask_id, junk=(5, 9), junk_id=1 << 40))
    return feats, {k: tables[k] for k in ("T300", "T3")}


@pytest.mark.parametrize("D", [16, 36, 132, 260, 1024, 3, 17, 65, 255])
def test_weighted_long_bags_and_weight_gradient_against_float64(D):
    """Float4 and scalar forms of every NV; masked ids (SUM_ID), out-of-range ids in front of / behind the bags and 5 % zero
    weights: dw there (and at every position no bag owns) is exactly 0 (``check`` asserts it where the reference's A is 0)."""
    for B in (B0, 1):
        feats, tables = _weighted_case(D, B, seed=77 * D + B)
        dY = _dy(B, 2 * D, seed=D + B)
        dev = Dev(feats, tables)
        bags = [f.bags(off_dtype=torch.int32) for f in feats]
        out = dev.run(bags, dY)
        assert header(dev.plan._long_ws) == expected_counts([f.lengths for f in feats])
        dws = {}
        for f, g in zip(feats, bags):
            dws[f.name], outside = f.dw_of(g)
            assert outside == 0, "%s: dw outside the bags is not zero" % f.name
            if f.pool == SUM_ID:
                masked = (f.flat == f.mask_id).cuda()
                assert int(masked.sum()) > 0 and int(torch.count_nonzero(dws[f.name][masked])) == 0
        check("weighted long D%d B%d" % (D, B), form(D) + " long bags", feats, tables, dY, out, dev.grads(), dws)


@pytest.mark.parametrize("D", [16, 132, 17])
def test_all_ones_weights_are_bit_equal_to_the_unweighted_long_call(D):
    feats, tables = _weighted_case(D, B0, seed=31 * D, ones=True)
    dY = _dy(B0, 2 * D, seed=D)
    dev = Dev(feats, tables)
    out_u = dev.run([f.bags(weighted=False) for f in feats], dY).detach().clone()
    assert header(dev.plan._long_ws)[0] > 0
    grads_u = {k: g.clone() for k, g in dev.grads().items()}
    out_w = dev.run([f.bags() for f in feats], dY).detach()
    assert torch.equal(out_w, out_u)
    for k, g in dev.grads().items():
        assert torch.equal(g, grads_u[k])


# ---- 5. malformed offsets that overflow the list ---------------------------------------------------------------------------
def test_overlapping_bags_overflow_the_list_and_stay_inside_out_and_workspace():
    """offsets = [0, nnz, 0, nnz, ...]: 20 bags of all 500 ids (10 000 ids of long bags over nnz = 500: the record list and
    the partial area fill up and the later bags are walked by their lane groups) and 20 decreasing pairs (empty bags)."""
    from recbox_amd import _lib, ops
    gen = torch.Generator().manual_seed(9)
    nnz, B, D, pad = 500, 40, 16, 4096
    table = make_table(300, D, gen)
    ids = torch.randint(0, 300, (nnz,), generator=gen)
    offsets = torch.tensor([0, nnz] * (B // 2) + [0], dtype=torch.int64)
    w = torch.nn.Parameter(table.clone().cuda())
    plan = ops.BagPlan([ops.BagSpec("h", D, 0, 0, _lib.POOL_SUM, 300)])
    bags = ops.Bags(ids.cuda(), offsets.cuda())
    old = ops.config.check_ids
    try:
        ops.config.check_ids = True
        with pytest.raises(IndexError):
            ops.embed_bags(plan, [bags], [w])
        ops.config.check_ids = False
        plan.bind_inputs([bags])
        plan.bind_params([w])
        need = _lib.lib.rbx_embed_csr_fwd_long_workspace_size(plan.arr, 1, B, T)
        big_out = torch.full((pad + B * D + pad,), 3.0, device="cuda")
        big_ws = torch.full((pad + need + pad,), 0x5A, dtype=torch.uint8, device="cuda")
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        out, ws = big_out[pad:pad + B * D], big_ws[pad:pad + need]
        _lib.check(_lib.lib.rbx_embed_csr_fwd_long(plan.arr, 1, B, T, out.data_ptr(), D, None, ws.data_ptr(), need,
                                                   status.data_ptr(), ops._stream()))
        torch.cuda.synchronize()
    finally:
        ops.config.check_ids = old
    assert int(status.item()) & _lib.STATUS_BAD_OFFSETS
    assert bool((big_out[:pad] == 3.0).all()) and bool((big_out[pad + B * D:] == 3.0).all())
    assert bool((big_ws[:pad] == 0x5A).all()) and bool((big_ws[pad + need:] == 0x5A).all())
    n_long, n_seg = header(ws)
    assert n_long >= 1 and n_seg >= 2                                        # some bags did take the long form
    got = out.view(B, D)
    rows = table[ids].double()
    want, A = rows.sum(0), rows.abs().sum(0)
    for b in range(0, B, 2):
        assert bound_ratio(got[b], want, A, max(C_BOUND, nnz + 2)) <= 1.0, "bag %d" % b
    assert int(torch.count_nonzero(got[1::2])) == 0


# ---- 6. one captured step ----------------------------------------------------------------------------------------------------
def test_long_bags_captured_in_one_graph_replay_on_new_contents_where_other_bags_are_long():
    from recbox_amd import ops
    gen = torch.Generator().manual_seed(3)
    D, V, B, nnz = 32, 5000, 257, 9000
    tables = {"T": (make_table(V, D, gen, pad=0), 0)}

    def contents(seed):
        g = torch.Generator().manual_seed(seed)
        cuts = torch.sort(torch.randint(0, nnz + 1, (B - 1,), generator=g)).values
        where = torch.randperm(B - 2, generator=g)[:6] + 1                   # six bags of several hundred ids, elsewhere per seed
        for k in where.tolist():
            cuts[k:] = torch.clamp(cuts[k:] + 400, max=nnz)
        offsets = torch.cat([torch.zeros(1, dtype=torch.int64), cuts, torch.tensor([nnz])])
        return torch.randint(0, V, (nnz,), generator=g), offsets

    feats = [Ragged("m", "T", "MEAN_ID", [], mask_id=0, eps=1e-8), Ragged("s", "T", "SUM", [])]
    dev = BagDevice(feats, tables)
    idx0, off0 = contents(1)
    idx1, off1 = contents(2)
    long0, long1 = (off0[1:] - off0[:-1]) >= T, (off1[1:] - off1[:-1]) >= T
    assert int(long0.sum()) > 0 and int(long1.sum()) > 0 and not torch.equal(long0, long1)
    indices, offsets = idx0.cuda(), off0.to(torch.int32).cuda()
    bags = [ops.Bags(indices, offsets)] * 2
    dY = _dy(B, 2 * D, 3).cuda()
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
        indices.copy_(idx1.cuda())
        offsets.copy_(off1.to(torch.int32).cuda())
        graph.replay()
        torch.cuda.synchronize()
        got_out, got_grad = out.detach().clone(), grad.clone()
        assert header(dev.plan._long_ws) == expected_counts([off1[1:] - off1[:-1]] * 2)
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
