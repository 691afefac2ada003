"""Per-sample weights of the ragged (CSR) lookup -- rbx_embed_csr_fwd_weighted / _sort_weighted / _bwd_weighted /
_weight_grad through ops.embed_bags -- against torch on the CPU in float64:

    F.embedding_bag(idx, W.double(), offsets, mode="sum", per_sample_weights=w.double(), include_last_offset=True)

and its autograd gradients for W and w, with the project's conventions applied by hand: a masked id (SUM_ID) enters the
reference with weight 0 and its dw is set to 0, the padding_idx row of dW is set to 0, ids outside every bag are cut off
(their dw is 0).  A comes from the same expression over |W|, |w|, |dY|.  Bound per element |got - want| <= C eps32 A + tiny:
forward C = max(C_BOUND, Lmax + 2), table gradient C = C_BOUND, weight gradient C = max(C_BOUND, D + 2); A = 0 means
exactly zero.  Every element of every output and gradient is compared."""
import ctypes

import pytest
import torch

from conftest import _note
from oracle.embed64 import C_BOUND, bound_ratio
from test_embed64_restatement import hot_row_batch, hot_row_dy, magnitudes, make_table
from test_gpu_embed_csr import _bag_ids, grid_bags
from test_gpu_embed_dims import SCALAR_NV1, SCALAR_NVN, VEC_NV1, VEC_NVN, form

pytestmark = pytest.mark.gpu
F = torch.nn.functional
SUM, SUM_ID, MEAN_ID = 1, 4, 3


class Feature(object):
    """One weighted feature on the CPU: ``ids`` (list of 1-D int64 tensors, one per bag), ``w`` flat float32 weights of the
    ids in order, the key of its table, its pool and mask id; ``junk`` ids (and weights) in front of / behind the bags."""

    def __init__(self, name, table, pool, ids, w, mask_id=None, junk=(0, 0), junk_id=0):
        self.name, self.table, self.pool, self.mask_id, self.junk = name, table, pool, mask_id, junk
        self.lengths = torch.tensor([t.numel() for t in ids], dtype=torch.int64)
        self.flat = torch.cat([torch.zeros(0, dtype=torch.int64)] + list(ids))
        self.w = w
        self.offsets = torch.zeros(len(ids) + 1, dtype=torch.int64)
        torch.cumsum(self.lengths, 0, out=self.offsets[1:])
        self.junk_id = junk_id

    def bags(self, weighted=True, requires_grad=True, idx_dtype=torch.int64, off_dtype=torch.int64):
        from recbox_amd import ops
        j0, j1 = self.junk
        flat = torch.cat([torch.full((j0,), self.junk_id, dtype=torch.int64), self.flat,
                          torch.full((j1,), self.junk_id, dtype=torch.int64)])
        w = None
        if weighted:
            w = torch.cat([torch.full((j0,), 3.0), self.w, torch.full((j1,), -2.0)]).cuda().requires_grad_(requires_grad)
        return ops.Bags(flat.to(idx_dtype).cuda(), (self.offsets + j0).to(off_dtype).cuda(), w)

    def dw_of(self, bags):
        """(the gradient of the weights inside the bags, the number of non-zeros outside them)."""
        g = bags.weights.grad
        j0 = self.junk[0]
        inside = g[j0:j0 + self.flat.numel()]
        return inside, int(torch.count_nonzero(g)) - int(torch.count_nonzero(inside))


def reference(feats, tables, dY):
    """float64 ``(out, A_out, {table: (gW, A_gW)}, {feature: (gw, A_gw)})`` of the features side by side in ``dY``'s columns."""
    def run(absolute):
        leaves = {k: (w.double().abs() if absolute else w.double()).clone().requires_grad_(True) for k, (w, _) in tables.items()}
        outs, wl = [], {}
        for f in feats:
            keep = torch.ones(f.flat.numel(), dtype=torch.float64)
            if f.pool == SUM_ID and f.mask_id is not None:
                keep = (f.flat != f.mask_id).double()
            wd = ((f.w.double().abs() if absolute else f.w.double()) * keep).requires_grad_(True)
            wl[f.name] = (wd, keep)
            if f.flat.numel() == 0:
                outs.append(torch.zeros(len(f.lengths), leaves[f.table].shape[1], dtype=torch.float64) + 0 * wd.sum())
                continue
            outs.append(F.embedding_bag(f.flat, leaves[f.table], f.offsets, mode="sum", per_sample_weights=wd,
                                        include_last_offset=True))
        out = torch.cat(outs, 1)
        out.backward(dY.double().abs() if absolute else dY.double())
        gW = {}
        for k, (w, pad) in tables.items():
            g = leaves[k].grad if leaves[k].grad is not None else torch.zeros_like(leaves[k])
            g = g.clone()
            if pad is not None:
                g[pad] = 0
            gW[k] = g
        gw = {n: (wd.grad if wd.grad is not None else torch.zeros_like(wd)) * keep for n, (wd, keep) in wl.items()}
        return out.detach(), gW, gw
    out, gW, gw = run(False)
    a_out, a_gW, a_gw = run(True)
    return out, a_out, {k: (gW[k], a_gW[k]) for k in gW}, {n: (gw[n], a_gw[n]) for n in gw}


def check(tag, label, feats, tables, dY, out, grads, dws, Lmax=None):
    """Every element of the outputs, of every table gradient and of every weight gradient against ``reference``."""
    want, a_out, gW, gw = reference(feats, tables, dY)
    Lmax = max([int(f.lengths.max()) if f.lengths.numel() else 0 for f in feats]) if Lmax is None else Lmax
    D = max(w.shape[1] for w, _ in tables.values())
    ratios = {"fwd": bound_ratio(out, want, a_out, max(C_BOUND, Lmax + 2))}
    for k, (g, a) in gW.items():
        if grads is not None and k in grads:
            ratios["dW " + k] = bound_ratio(grads[k], g, a)
            assert int(torch.count_nonzero(grads[k].detach().cpu()[a == 0])) == 0
    for n, (g, a) in gw.items():
        if dws is not None and n in dws:
            ratios["dw " + n] = bound_ratio(dws[n], g, a, max(C_BOUND, D + 2))
            assert int(torch.count_nonzero(dws[n].detach().cpu()[a == 0])) == 0
    print("%s [%s]: %s" % (tag, label, ", ".join("%s %.3g" % kv for kv in sorted(ratios.items()))))
    _note("%s weighted forward (err / bound)" % label, ratios["fwd"], 1.0)
    _note("%s weighted table gradient (err / bound)" % label, max([v for k, v in ratios.items() if k.startswith("dW")] or [0.0]), 1.0)
    _note("%s weight gradient (err / bound)" % label, max([v for k, v in ratios.items() if k.startswith("dw ")] or [0.0]), 1.0)
    worst = max(ratios.items(), key=lambda kv: kv[1])
    assert worst[1] <= 1.0, "%s: %s error is %.3g x the bound" % (tag, worst[0], worst[1])


class Dev(object):
    """Tables as parameters on the GPU and the BagPlan of the features (slots side by side)."""

    def __init__(self, feats, tables, pools=None):
        from recbox_amd import ops
        self.feats, self.keys = feats, list(tables)
        self.params = {k: torch.nn.Parameter(w.clone().cuda()) for k, (w, _) in tables.items()}
        specs, off = [], 0
        for f in feats:
            w, pad = tables[f.table]
            specs.append(ops.BagSpec(f.name, w.shape[1], off, self.keys.index(f.table), f.pool, w.shape[0], padding_idx=pad,
                                     mask_id=f.mask_id))
            off += w.shape[1]
        self.plan, self.width = ops.BagPlan(specs), off

    def plist(self):
        return [self.params[k] for k in self.keys]

    def run(self, bags, dY=None, retain_graph=False):
        from recbox_amd import ops
        for p in self.params.values():
            p.grad = None
        out = ops.embed_bags(self.plan, bags, self.plist())
        if dY is not None:
            out.backward(dY.cuda(), retain_graph=retain_graph)
        torch.cuda.synchronize()
        return out

    def grads(self):
        return {k: (p.grad if p.grad is not None else torch.zeros_like(p)) for k, p in self.params.items()}


def _weights(n, gen, zero_frac=0.0):
    w = magnitudes((n,), gen) * 2.0                                         # both signs, |w| in [0.1, 2]
    if zero_frac:
        w[torch.rand(n, generator=gen) < zero_frac] = 0.0
    return w


def _dy(B, width, seed):
    return magnitudes((B, width), torch.Generator().manual_seed(seed))


def _grid(D, B, seed):
    """The SUM and SUM_ID features of test_gpu_embed_csr's grid (tables of 300 and 3 rows, bags of 0 .. 40 ids plus five of
    300 .. 699, ~10 % masked ids in the SUM_ID bags) with random weights, 5 % of them exactly zero."""
    ragged, tables = grid_bags(D, B, seed=seed, big=1000)
    gen = torch.Generator().manual_seed(seed + 1)
    feats = []
    for r in ragged:
        if r.pool in ("SUM", "SUM_ID"):
            n = int(r.lengths.sum())
            feats.append(Feature(r.name, r.table, SUM if r.pool == "SUM" else SUM_ID, r.ids, _weights(n, gen, 0.05), r.mask_id,
                                 junk=(5, 9), junk_id=1 << 40))
    return feats, {k: tables[k] for k in ("T300", "T3")}


# ---- the dim grid -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", VEC_NV1 + VEC_NVN + SCALAR_NV1 + SCALAR_NVN)
def test_weighted_bags_grid_of_dims_against_float64(D):
    """Every lane-group form, float4 and scalar; B = 2053 and B = 1; int64 indices with int32 offsets; OUT-OF-RANGE ids (and
    weights) in front of offsets[0] and behind offsets[B] that nothing may read and whose dw is exactly 0."""
    for B in (2053, 1):
        feats, tables = _grid(D, B, seed=1000 * D + B)
        dY = _dy(B, 2 * D, seed=D + B)
        dev = Dev(feats, tables)
        bags = [f.bags(off_dtype=torch.int32) for f in feats]
        out = dev.run(bags, dY)
        dws = {}
        for f, g in zip(feats, bags):
            dws[f.name], outside = f.dw_of(g)
            assert outside == 0, "%s: dw outside the bags is not zero" % f.name
        check("weighted grid D%d B%d" % (D, B), form(D) + " bags", feats, tables, dY, out, dev.grads(), dws)
        assert int(torch.count_nonzero(dev.grads()["T300"][0])) == 0        # the padding_idx row


@pytest.mark.parametrize("D", VEC_NV1 + VEC_NVN + SCALAR_NV1 + SCALAR_NVN)
def test_all_ones_weights_are_bit_equal_to_the_unweighted_call(D):
    B = 1031
    feats, tables = _grid(D, B, seed=77 * D)
    for f in feats:
        f.w = torch.ones_like(f.w)
    dY = _dy(B, 2 * D, seed=D)
    dev = Dev(feats, tables)
    out_u = dev.run([f.bags(weighted=False) for f in feats], dY).detach().clone()
    grads_u = {k: g.clone() for k, g in dev.grads().items()}
    out_w = dev.run([f.bags() for f in feats], dY).detach()
    for k, g in dev.grads().items():
        assert torch.equal(g, grads_u[k]), "D%d: table gradient of %s differs from the unweighted call's" % (D, k)
    assert torch.equal(out_w, out_u)


# ---- hot rows, repeatability ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [16, 132, 256])
def test_weighted_hot_rows_against_float64_and_two_backwards_over_one_sort(D):
    ids, sign = hot_row_batch(100000, seed=16, L=7)
    gen = torch.Generator().manual_seed(D + 5)
    B = ids.shape[0]
    lengths = torch.randint(1, 8, (B,), generator=gen)
    lengths[(ids == 7).any(1)] = 7
    bag_ids = [ids[b, :int(n)] for b, n in enumerate(lengths.tolist())]
    w = (0.5 + torch.rand(int(lengths.sum()), generator=gen)).float()       # positive: the hot row's terms cannot cancel
    feat = Feature("hot", "T", SUM_ID, bag_ids, w, mask_id=0)
    tables = {"T": (make_table(1000, D, gen), None)}
    dY = hot_row_dy(sign, D, gen)
    dev = Dev([feat], tables)
    bags = [feat.bags()]
    out = dev.run(bags, dY, retain_graph=True)
    dw = bags[0].weights.grad.clone()
    check("weighted hot rows D%d" % D, form(D) + " bags hot rows", [feat], tables, dY, out, dev.grads(), {"hot": dw}, Lmax=7)
    first = dev.grads()["T"].clone()
    dev.params["T"].grad, bags[0].weights.grad = None, None
    out.backward(dY.cuda())
    torch.cuda.synchronize()
    assert torch.equal(dev.grads()["T"], first)
    assert torch.equal(bags[0].weights.grad, dw)


# ---- edges ------------------------------------------------------------------------------------------------------------------
def _table(D=16, V=300, seed=3, pad=0):
    gen = torch.Generator().manual_seed(seed)
    return gen, {"T": (make_table(V, D, gen, pad=None), pad)}              # the padding row holds values: its dw is not zero


def test_all_bags_empty_and_a_batch_of_zero_bags():
    from recbox_amd import ops
    gen, tables = _table()
    B = 77
    feat = Feature("h", "T", SUM, [torch.zeros(0, dtype=torch.int64)] * B, torch.zeros(0), junk=(3, 4), junk_id=5)
    dev = Dev([feat], tables)
    for f in (feat, Feature("h", "T", SUM, [torch.zeros(0, dtype=torch.int64)] * B, torch.zeros(0))):
        bags = [f.bags()]
        out = dev.run(bags, _dy(B, 16, 1))
        assert int(torch.count_nonzero(out)) == 0 and int(torch.count_nonzero(dev.grads()["T"])) == 0
        assert int(torch.count_nonzero(bags[0].weights.grad)) == 0
    w = torch.tensor([1.0, 2.0, 3.0], device="cuda", requires_grad=True)
    bags = ops.Bags(torch.tensor([4, 5, 6]).cuda(), torch.tensor([1]).cuda(), w)
    out = ops.embed_bags(dev.plan, [bags], dev.plist())
    assert tuple(out.shape) == (0, 16)
    out.sum().backward()
    torch.cuda.synchronize()
    assert int(torch.count_nonzero(w.grad)) == 0 and tuple(w.grad.shape) == (3,)


def test_offsets_inside_the_index_array_leave_dw_outside_the_bags_exactly_zero():
    gen, tables = _table()
    B = 300
    lengths = torch.randint(0, 30, (B,), generator=gen)
    feat = Feature("h", "T", SUM, _bag_ids(300, lengths, gen, lo=0), _weights(int(lengths.sum()), gen), junk=(11, 23), junk_id=7)
    dev = Dev([feat], tables)
    dY = _dy(B, 16, 2)
    bags = [feat.bags()]
    out = dev.run(bags, dY)
    dw, outside = feat.dw_of(bags[0])
    assert outside == 0
    check("offsets[0] > 0, offsets[B] < nnz", form(16) + " bags edges", [feat], tables, dY, out, dev.grads(), {"h": dw})


def test_every_id_masked():
    gen, tables = _table()
    B = 257
    lengths = torch.randint(0, 30, (B,), generator=gen)
    n = int(lengths.sum())
    feat = Feature("s", "T", SUM_ID, [torch.zeros(int(k), dtype=torch.int64) for k in lengths], _weights(n, gen), mask_id=0)
    dev = Dev([feat], tables)
    bags = [feat.bags()]
    out = dev.run(bags, _dy(B, 16, 1))
    assert int(torch.count_nonzero(out)) == 0 and int(torch.count_nonzero(dev.grads()["T"])) == 0
    assert int(torch.count_nonzero(bags[0].weights.grad)) == 0


def test_padding_idx_id_is_read_and_weighted_gets_a_dw_and_a_zero_table_gradient_row():
    gen, tables = _table(pad=0)
    B = 400
    lengths = torch.randint(1, 20, (B,), generator=gen)
    ids = _bag_ids(300, lengths, gen, lo=0, masked_frac=0.2)                # 20 % of the ids are 0 = the padding_idx row
    feat = Feature("h", "T", SUM, ids, _weights(int(lengths.sum()), gen, zero_frac=0.1))   # zero and negative weights too
    dev = Dev([feat], tables)
    dY = _dy(B, 16, 4)
    bags = [feat.bags()]
    out = dev.run(bags, dY)
    dw = bags[0].weights.grad
    check("padding_idx id", form(16) + " bags edges", [feat], tables, dY, out, dev.grads(), {"h": dw})
    assert int(torch.count_nonzero(dev.grads()["T"][0])) == 0
    at_pad = (feat.flat == 0).cuda()
    assert int(at_pad.sum()) > 100 and int(torch.count_nonzero(dw[at_pad])) == int(at_pad.sum())


@pytest.mark.parametrize("D", [16, 132])
def test_one_weighted_bag_holds_every_id(D):
    gen, tables = _table(D=D)
    n = 5000
    feat = Feature("s", "T", SUM, [torch.randint(0, 300, (n,), generator=gen)], _weights(n, gen))
    dev = Dev([feat], tables)
    dY = _dy(1, D, 2)
    bags = [feat.bags()]
    out = dev.run(bags, dY)
    check("one bag of %d ids D%d" % (n, D), form(D) + " one bag", [feat], tables, dY, out, dev.grads(), {"s": bags[0].weights.grad})


# ---- bad input goes through the status word ---------------------------------------------------------------------------------
def test_out_of_range_ids_and_malformed_offsets_raise_and_leave_the_well_formed_bags_correct():
    from recbox_amd import ops
    gen, tables = _table()
    B = 200
    lengths = torch.randint(0, 12, (B,), generator=gen)
    lengths[10:14] = torch.tensor([6, 5, 7, 4])
    ids = _bag_ids(300, lengths, gen)
    nnz = int(lengths.sum())
    w = _weights(nnz, gen)
    feats = [Feature(n, "T", SUM, ids, w) for n in ("good", "decreasing", "beyond", "bad_id")]
    dev = Dev(feats, tables)
    buf = torch.full((nnz + 4000,), 7, dtype=torch.int64, device="cuda")    # indices / weights: views into larger buffers
    wbuf = torch.full((nnz + 4000,), 0.5, device="cuda")
    flat, wflat = buf[2000:2000 + nnz], wbuf[2000:2000 + nnz]
    flat.copy_(torch.cat(ids))
    wflat.copy_(w)
    offsets = feats[0].offsets
    dec, bey = offsets.clone(), offsets.clone()
    dec[12] = dec[11] - 3
    bey[B] = nnz + 7
    wrong = flat.clone()
    first_of_bag_50 = int(offsets[50])
    assert lengths[50] > 0
    wrong[first_of_bag_50] = 300                                            # vocab: one past the last row
    clean = [ops.Bags(flat, offsets.cuda(), wflat)] * 4
    with torch.no_grad():
        want = ops.embed_bags(dev.plan, clean, dev.plist())
    old = ops.config.check_ids
    try:
        for k, bad_bags in ((1, ops.Bags(flat, dec.cuda(), wflat)), (2, ops.Bags(flat, bey.cuda(), wflat)),
                            (3, ops.Bags(wrong, offsets.cuda(), wflat))):
            ops.config.check_ids = True
            call = list(clean)
            call[k] = bad_bags
            with pytest.raises(IndexError):
                ops.embed_bags(dev.plan, call, dev.plist())
        ops.config.check_ids = False
        try:
            ops.check_deferred_ids()
        except IndexError:
            pass
        bad = [clean[0], ops.Bags(flat, dec.cuda(), wflat), ops.Bags(flat, bey.cuda(), wflat), ops.Bags(wrong, offsets.cuda(), wflat)]
        out = ops.embed_bags(dev.plan, bad, dev.plist())
        out.backward(_dy(B, 64, 9).cuda())                                  # sort + reduce clamp the same way: nothing faults
        with pytest.raises(IndexError):
            ops.check_deferred_ids()
    finally:
        ops.config.check_ids = old
    torch.cuda.synchronize()
    out, D = out.detach(), 16
    assert torch.equal(out[:, :D], want[:, :D])
    intact = torch.ones(B, dtype=torch.bool)
    intact[11:13] = False
    assert torch.equal(out[intact, D:2 * D], want[intact, D:2 * D])
    assert int(torch.count_nonzero(out[11, D:2 * D])) == 0
    assert torch.equal(out[:B - 1, 2 * D:3 * D], want[:B - 1, 2 * D:3 * D])
    rest = torch.ones(B, dtype=torch.bool)
    rest[50] = False
    assert torch.equal(out[rest, 3 * D:], want[rest, 3 * D:])


# ---- mixed calls, frozen parts ------------------------------------------------------------------------------------------------
def test_weighted_and_unweighted_descriptor_share_a_table():
    gen, tables = _table(D=32, V=500)
    B = 700
    la, lb = torch.randint(0, 25, (B,), generator=gen), torch.randint(0, 25, (B,), generator=gen)
    fa = Feature("plain", "T", SUM, _bag_ids(500, la, gen, lo=0), torch.ones(int(la.sum())))
    fb = Feature("scored", "T", SUM, _bag_ids(500, lb, gen, lo=0), _weights(int(lb.sum()), gen))
    dY = _dy(B, 64, 3)
    dev = Dev([fa, fb], tables)
    bags = [fa.bags(weighted=False), fb.bags()]
    out = dev.run(bags, dY)
    check("mixed call", form(32) + " bags mixed", [fa, fb], tables, dY, out, dev.grads(), {"scored": bags[1].weights.grad})
    alone = Dev([fa], tables)
    out_a = alone.run([fa.bags(weighted=False)], dY[:, :32])
    assert torch.equal(out.detach()[:, :32], out_a.detach())


def test_frozen_table_with_trainable_weights_and_the_reverse():
    gen, tables = _table(D=20, V=400)
    B = 500
    lengths = torch.randint(0, 25, (B,), generator=gen)
    feat = Feature("h", "T", SUM, _bag_ids(400, lengths, gen, lo=0), _weights(int(lengths.sum()), gen))
    dY = _dy(B, 20, 3)
    dev = Dev([feat], tables)
    dev.params["T"].requires_grad_(False)
    bags = [feat.bags()]
    out = dev.run(bags, dY)
    assert dev.params["T"].grad is None
    check("frozen table", form(20) + " bags frozen table", [feat], tables, dY, out, None, {"h": bags[0].weights.grad})
    dev.params["T"].requires_grad_(True)
    bags = [feat.bags(requires_grad=False)]
    out = dev.run(bags, dY)
    assert bags[0].weights.grad is None
    check("frozen weights", form(20) + " bags frozen weights", [feat], tables, dY, out, dev.grads(), None)


# ---- one captured step ------------------------------------------------------------------------------------------------------
def test_weighted_forward_backward_and_weight_gradient_captured_in_one_graph():
    from recbox_amd import ops
    gen, tables = _table(D=32, V=5000)
    B, nnz = 513, 9000

    def contents(seed):
        g = torch.Generator().manual_seed(seed)
        cuts = torch.sort(torch.randint(0, nnz + 1, (B - 1,), generator=g)).values
        offsets = torch.cat([torch.zeros(1, dtype=torch.int64), cuts, torch.tensor([nnz])])
        return torch.randint(0, 5000, (nnz,), generator=g), offsets, _weights(nnz, g)

    dev = Dev([Feature("s", "T", SUM, [], torch.zeros(0))], tables)
    idx0, off0, w0 = contents(1)
    indices, offsets = idx0.cuda(), off0.to(torch.int32).cuda()
    weights = w0.cuda().requires_grad_(True)
    bags = [ops.Bags(indices, offsets, weights)]
    dY = _dy(B, 32, 3).cuda()
    table = dev.params["T"]
    old = ops.config.check_ids
    try:
        ops.config.check_ids = False
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                table.grad, weights.grad = None, None
                ops.embed_bags(dev.plan, bags, dev.plist()).backward(dY)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        table.grad, weights.grad = None, None
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = ops.embed_bags(dev.plan, bags, dev.plist())
            out.backward(dY)
        grad, dw = table.grad, weights.grad
        idx1, off1, w1 = contents(2)
        indices.copy_(idx1.cuda())
        offsets.copy_(off1.to(torch.int32).cuda())
        with torch.no_grad():
            weights.copy_(w1.cuda())
        graph.replay()
        torch.cuda.synchronize()
        got = out.detach().clone(), grad.clone(), dw.clone()
        table.grad = None
        w_eager = w1.cuda().requires_grad_(True)
        want_out = ops.embed_bags(dev.plan, [ops.Bags(idx1.cuda(), off1.cuda(), w_eager)], dev.plist())
        want_out.backward(dY)
        torch.cuda.synchronize()
        ops.check_deferred_ids()
    finally:
        ops.config.check_ids = old
    assert torch.equal(got[0], want_out.detach())
    assert torch.equal(got[1], table.grad) and torch.equal(got[2], w_eager.grad)
    assert int(torch.count_nonzero(got[1])) > 0 and int(torch.count_nonzero(got[2])) > 0


# ---- refusals -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pool", [MEAN_ID, 2])
def test_weighted_mean_pools_are_refused_by_the_c_calls_and_nothing_is_written(pool):
    from recbox_amd import _lib, ops
    gen, tables = _table()
    table = tables["T"][0].cuda()
    bags = ops.Bags(torch.randint(0, 300, (40,), generator=gen).cuda(), torch.tensor([0, 7, 40]).cuda())
    plan = ops.BagPlan([ops.BagSpec("h", 16, 0, 0, pool, 300, eps=1e-8)])
    plan.bind_inputs([bags])
    plan.bind_params([table], [None])
    w = torch.ones(40, device="cuda")
    out = torch.full((2, 16), 5.0, device="cuda")
    dw = torch.full((40,), 5.0, device="cuda")
    warr = (ctypes.c_void_p * 1)(w.data_ptr())
    dwarr = (ctypes.c_void_p * 1)(dw.data_ptr())
    lib = _lib.lib
    assert lib.rbx_embed_csr_fwd_weighted(plan.arr, 1, 2, warr, out.data_ptr(), 16, None, None) == _lib.RBX_ERR_UNSUPPORTED
    assert lib.rbx_embed_csr_weight_grad(plan.arr, 1, 2, out.data_ptr(), 16, dwarr, None, None) == _lib.RBX_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out == 5.0).all()) and bool((dw == 5.0).all())
    with pytest.raises(NotImplementedError):
        ops.embed_bags(plan, [ops.Bags(bags.indices, bags.offsets, w)], [table])


# ---- the rechub layer -------------------------------------------------------------------------------------------------------
def test_rechub_embedding_layer_takes_weighted_bags_for_sum_pooled_sequence_features():
    from recbox_amd import ops
    from recbox_amd.rechub.basic.features import SequenceFeature, SparseFeature
    from recbox_amd.rechub.basic.layers import EmbeddingLayer
    from test_embed64_restatement import history
    gen = torch.Generator().manual_seed(11)
    B, L, D = 900, 20, 16
    feats = [SparseFeature("a", 50, D), SequenceFeature("hist_m", 300, D, pooling="mean", padding_idx=0),
             SequenceFeature("hist_c", 700, D, pooling="sum", padding_idx=0)]
    layer = EmbeddingLayer(feats).cuda()
    wt = make_table(layer.embed_dict["hist_c"].num_embeddings, D, gen)
    layer.embed_dict["hist_c"].weight.data.copy_(wt)
    pad = layer.embed_dict["hist_c"].padding_idx
    ids = history(700, B, L, gen)
    scores = _weights(B * L, gen).view(B, L)
    x = {"a": torch.randint(0, 50, (B,), generator=gen).cuda(), "hist_m": ops.bags_from_padded(history(300, B, L, gen).cuda(), 0)}
    dY = _dy(B, 3 * D, 5)

    def run(weights, features):
        for m in layer.embed_dict.values():
            m.weight.grad = None
        bags = ops.bags_from_padded(ids.cuda(), 0, weights)
        if bags.weights is not None:
            bags.weights.requires_grad_(True)
        out = layer(dict(x, hist_c=bags), features, squeeze_dim=True)
        out.backward(dY.cuda()[:, :out.shape[1]])
        torch.cuda.synchronize()
        return out.detach(), layer.embed_dict["hist_c"].weight.grad.clone(), bags

    out, grad, bags = run(scores.cuda(), feats)                              # (the unweighted mean bags beside it: two calls)
    keep = ids != 0
    feat = Feature("hist_c", "T", SUM_ID, [ids[b][keep[b]] for b in range(B)], scores[keep], mask_id=0)
    check("rechub layer, weighted sum", form(D) + " layer weighted bags", [feat], {"T": (wt, pad)}, dY[:, 2 * D:], out[:, 2 * D:],
          {"T": grad}, {"hist_c": bags.weights.grad})
    pair = [feats[0], feats[2]]                                              # one bag descriptor either way: the same sort
    out_1, grad_1, _ = run(torch.ones(B, L, device="cuda"), pair)
    out_u, grad_u, _ = run(None, pair)
    assert torch.equal(out_1, out_u) and torch.equal(grad_1, grad_u)
    mean = [SequenceFeature("dwell", 300, D, pooling="mean", padding_idx=0)]
    layer_m = EmbeddingLayer(mean).cuda()
    with pytest.raises(NotImplementedError, match="dwell"):
        layer_m({"dwell": bags}, mean, squeeze_dim=True)
