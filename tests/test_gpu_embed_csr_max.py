"""The max pool of the ragged (CSR) lookup (POOL_MAX, rbx_embed_csr_fwd_max / rbx_embed_csr_bwd_max) against torch's CPU
``F.embedding_bag(mode="max")``.  A max selects and never rounds, so outputs and argpos are compared with ``torch.equal``.
Table gradients are held to the project's bound against a float64 reference written here: torch CPU autograd over
``W.double()`` with the padding row zeroed by hand, ``A`` the same gradient with ``|dY|`` upstream (the gradient is linear
in dY for a fixed selection, so that is the sum of the absolute terms), ``|got - want| <= C_BOUND eps32 A`` for every
element and exactly 0 where ``A == 0``."""
import pytest
import torch

from conftest import _note
from oracle.embed64 import C_BOUND, bound_ratio
from test_embed64_restatement import magnitudes, make_table
from test_gpu_embed_csr import _bag_ids, grid_bags
from test_gpu_embed_dims import SCALAR_NV1, SCALAR_NVN, VEC_NV1, VEC_NVN, form

pytestmark = pytest.mark.gpu
F = torch.nn.functional
JUNK_ID = 1 << 40                                          # out of every range: nothing may read the ids outside the bags


class Feat(object):
    """One max-pooled feature on the CPU: the ids of its bags, the key of its table, its mask id and the ``junk`` ids in
    front of the first and behind the last bag."""

    def __init__(self, name, table, ids, mask=None, junk=(0, 0)):
        self.name, self.table, self.mask, self.junk = name, table, mask, junk
        self.lengths = torch.tensor([t.numel() for t in ids], dtype=torch.int64)
        self.flat = torch.cat([torch.zeros(0, dtype=torch.int64)] + list(ids))
        self.offsets = torch.zeros(len(ids) + 1, dtype=torch.int64)
        torch.cumsum(self.lengths, 0, out=self.offsets[1:])

    def full(self):
        j0, j1 = self.junk
        return torch.cat([torch.full((j0,), JUNK_ID, dtype=torch.int64), self.flat, torch.full((j1,), JUNK_ID, dtype=torch.int64)])

    def bags(self, idx_dtype=torch.int64, off_dtype=torch.int64):
        from recbox_amd import ops
        return ops.Bags(self.full().to(idx_dtype).cuda(), (self.offsets + self.junk[0]).to(off_dtype).cuda())


def cpu_max(idx, W, offsets, mask=None):
    if idx.numel() == 0:
        return torch.zeros(offsets.numel() - 1, W.shape[1], dtype=W.dtype) + 0 * W.sum()
    return F.embedding_bag(idx, W, offsets, mode="max", include_last_offset=True, padding_idx=mask)


def reference(feats, tables, dY):
    """(float32 out of torch's CPU kernel, {table: (float64 gradient, A)}) of the features side by side in dY's columns."""
    out32 = torch.cat([cpu_max(f.flat, tables[f.table][0], f.offsets, f.mask) for f in feats], 1)
    leaves = {k: w.double().clone().requires_grad_(True) for k, (w, _) in tables.items()}
    out = torch.cat([cpu_max(f.flat, leaves[f.table], f.offsets, f.mask) for f in feats], 1)
    keys = list(leaves)
    g = torch.autograd.grad(out, [leaves[k] for k in keys], dY.double(), retain_graph=True, allow_unused=True)
    a = torch.autograd.grad(out, [leaves[k] for k in keys], dY.double().abs(), allow_unused=True)
    grads = {}
    for k, gk, ak in zip(keys, g, a):
        gk = torch.zeros_like(leaves[k]) if gk is None else gk.clone()
        ak = torch.zeros_like(leaves[k]) if ak is None else ak.clone()
        pad = tables[k][1]
        if pad is not None:
            gk[pad], ak[pad] = 0, 0
        grads[k] = (gk, ak)
    return out32, grads


class Dev(object):
    def __init__(self, feats, tables):
        from recbox_amd import ops
        self.feats, self.keys = feats, list(tables)
        self.params = {k: torch.nn.Parameter(w.clone().cuda()) for k, (w, _) in tables.items()}
        specs, off = [], 0
        for f in feats:
            w, pad = tables[f.table]
            specs.append(ops.BagSpec(f.name, w.shape[1], off, self.keys.index(f.table), ops.POOL_MAX, w.shape[0], padding_idx=pad,
                                     mask_id=f.mask))
            off += w.shape[1]
        self.plan, self.width = ops.BagPlan(specs), off

    def plist(self):
        return [self.params[k] for k in self.keys]

    def run(self, bags, dY=None):
        """(out, argpos, {table: grad}) on the CPU."""
        from recbox_amd import ops
        for p in self.params.values():
            p.grad = None
        out = ops.embed_bags(self.plan, bags, self.plist())
        argpos = out.grad_fn.argpos
        if dY is not None:
            out.backward(dY.cuda())
        torch.cuda.synchronize()
        grads = {k: (p.grad if p.grad is not None else torch.zeros_like(p)).detach().cpu() for k, p in self.params.items()}
        return out.detach().cpu(), argpos.cpu(), grads


def check_argpos(f, W, out, argpos):
    """argpos of one feature, directly: -1 exactly where the bag has no usable id; otherwise the row it names holds the
    output and no lower usable position of the bag attains it."""
    idx, j0 = f.full(), f.junk[0]
    V = W.shape[0]
    for b in range(len(f.lengths)):
        lo, hi = int(f.offsets[b]) + j0, int(f.offsets[b + 1]) + j0
        pos = torch.arange(lo, hi)
        ids = idx[lo:hi]
        ok = (ids >= 0) & (ids < V)
        if f.mask is not None:
            ok &= ids != f.mask
        pos, ids = pos[ok], ids[ok]
        if pos.numel() == 0:
            assert bool((argpos[b] == -1).all()) and int(torch.count_nonzero(out[b])) == 0, "bag %d of %s" % (b, f.name)
            continue
        rows = W[ids]
        best = rows.max(0).values
        first = torch.where(rows == best, pos[:, None], torch.tensor(1 << 60)).min(0).values
        assert torch.equal(out[b], best), "bag %d of %s: out" % (b, f.name)
        assert torch.equal(argpos[b].long(), first), "bag %d of %s: argpos" % (b, f.name)


def check(tag, label, feats, tables, dY, out, argpos, grads):
    want, gW = reference(feats, tables, dY)
    assert torch.equal(out, want), "%s: out differs from torch's CPU max" % tag
    off = 0
    for f in feats:
        W = tables[f.table][0]
        D = W.shape[1]
        check_argpos(f, W, out[:, off:off + D], argpos[:, off:off + D])
        off += D
    ratios = {}
    for k, (g, a) in gW.items():
        ratios[k] = bound_ratio(grads[k], g, a)
        assert int(torch.count_nonzero(grads[k][a == 0])) == 0, "%s: dW %s is not exactly 0 where A == 0" % (tag, k)
    print("%s [%s]: %s" % (tag, label, ", ".join("dW %s %.3g" % kv for kv in sorted(ratios.items()))))
    _note("%s max table gradient (err / bound)" % label, max(ratios.values()), 1.0)
    worst = max(ratios.items(), key=lambda kv: kv[1])
    assert worst[1] <= 1.0, "%s: dW %s error is %.3g x the bound" % (tag, worst[0], worst[1])


def _dy(B, width, seed):
    return magnitudes((B, width), torch.Generator().manual_seed(seed))


# ---- 1. every lane-group form ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", VEC_NV1 + VEC_NVN + SCALAR_NV1 + SCALAR_NVN)
def test_max_bags_grid_of_dims_against_torch_cpu(D):
    """Four max features in one call (two share the 300-row table, one pools 3 rows: long runs in the reduce), B = 37 --
    no multiple of a groups-per-wave count -- bags of 0 .. 40 ids plus five of 300 .. 699, ~10 % masked ids, out-of-range
    junk ids in front of and behind the bags; int64 ids with int32 offsets as well."""
    B = 37
    ragged, tables = grid_bags(D, B, seed=300 + D, big=1000)
    feats = [Feat(r.name, r.table, r.ids, r.mask_id, junk=(5, 9)) for r in ragged]
    dY = _dy(B, 4 * D, D)
    dev = Dev(feats, tables)
    for idt, odt in ((torch.int64, torch.int64), (torch.int64, torch.int32)):
        out, argpos, grads = dev.run([f.bags(idt, odt) for f in feats], dY)
        check("max grid D=%d" % D, form(D) + " bags max", feats, tables, dY, out, argpos, grads)


# ---- 2. ties --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [4, 8, 64, 10, 3])
def test_ties_go_to_the_lowest_position_like_torch(D):
    """Table entries from {-1, 0, 1}: every column of every bag ties between different rows, ids repeat inside bags; dY of
    small integers makes every gradient sum exact in fp32, so all three results equal torch's bit for bit.  D = 4, 8 and 3:
    narrow rows, R > 1 sub-groups per lane group; 64: one float4 group; 10: scalar."""
    gen = torch.Generator().manual_seed(D)
    V, B = 12, 101
    W = torch.randint(-1, 2, (V, D), generator=gen).float()
    lengths = torch.randint(0, 30, (B,), generator=gen)
    lengths[7] = 150
    f = Feat("t", "T", _bag_ids(V, lengths, gen, lo=0), junk=(3, 2))
    tables = {"T": (W, None)}
    dY = torch.randint(-3, 4, (B, D), generator=gen).float()
    out, argpos, grads = Dev([f], tables).run([f.bags()], dY)
    leaf = W.clone().requires_grad_(True)
    want = cpu_max(f.flat, leaf, f.offsets)
    want.backward(dY)
    assert torch.equal(out, want.detach())
    check_argpos(f, W, out, argpos)
    assert torch.equal(grads["T"], leaf.grad)


def test_torch_tie_rule_is_first_occurrence():
    """The rule the contract rests on, on this torch: ids [1, 0, 2, 0] over a column holding 2, 5, 5, 5 -> id 0."""
    W = torch.tensor([[5.0], [2.0], [5.0]]).cuda()
    p = torch.nn.Parameter(W)
    from recbox_amd import ops
    out = ops.embed_bags([ops.BagSpec("t", 1, 0, 0, ops.POOL_MAX, 3)],
                         [ops.Bags(torch.tensor([1, 0, 2, 0]).cuda(), torch.tensor([0, 4]).cuda())], [p])
    out.backward(torch.ones(1, 1).cuda())
    assert out.item() == 5.0 and out.grad_fn.argpos.item() == 1
    assert p.grad.cpu().flatten().tolist() == [1.0, 0.0, 0.0]
    leaf = W.cpu().clone().requires_grad_(True)
    cpu_max(torch.tensor([1, 0, 2, 0]), leaf, torch.tensor([0, 4])).backward(torch.ones(1, 1))
    assert leaf.grad.flatten().tolist() == [1.0, 0.0, 0.0]


# ---- 3. an all-negative table: the zero rows are zeros because nothing was taken, not because 0 won ----------------------------
@pytest.mark.parametrize("D", [16, 5])
def test_all_negative_table_bags_without_a_usable_id_are_zero_rows_with_argpos_minus_one(D):
    from recbox_amd import ops
    gen = torch.Generator().manual_seed(5)
    V, B = 50, 40
    W = -1.0 - torch.rand(V, D, generator=gen)
    lengths = torch.randint(1, 9, (B,), generator=gen)
    lengths[3] = 0
    ids = _bag_ids(V, lengths, gen, lo=1)
    ids[8] = torch.zeros(6, dtype=torch.int64)              # masked ids only
    ids[20] = torch.tensor([V, V + 7, -1, 1 << 33])         # out-of-range ids only
    f = Feat("n", "T", ids, mask=0)
    tables = {"T": (W, 0)}
    dY = _dy(B, D, 2)
    dev = Dev([f], tables)
    old = ops.config.check_ids
    try:
        ops.config.check_ids = True
        with pytest.raises(IndexError):
            dev.run([f.bags()], dY)
        ops.config.check_ids = False
        try:
            ops.check_deferred_ids()
        except IndexError:
            pass
        out, argpos, grads = dev.run([f.bags()], dY)
        with pytest.raises(IndexError):
            ops.check_deferred_ids()
    finally:
        ops.config.check_ids = old
    for b in (3, 8, 20):
        assert int(torch.count_nonzero(out[b])) == 0 and bool((argpos[b] == -1).all())
    rest = torch.ones(B, dtype=torch.bool)
    rest[[3, 8, 20]] = False
    assert bool((out[rest] < 0).all()) and bool((argpos[rest] >= 0).all())
    clean = Feat("n", "T", [t if b != 20 else t[:0] for b, t in enumerate(ids)], mask=0)
    want, gW = reference([clean], tables, dY)
    assert torch.equal(out, want)
    check_argpos(f, W, out, argpos)
    g, a = gW["T"]
    assert bound_ratio(grads["T"], g, a) <= 1.0 and int(torch.count_nonzero(grads["T"][a == 0])) == 0


# ---- 4. mask_id / padding_idx ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [32, 7])
def test_masked_id_is_left_out_even_when_its_row_holds_the_maximum(D):
    gen = torch.Generator().manual_seed(11)
    V, B, P = 40, 60, 6
    W = magnitudes((V, D), gen)
    W[P] = 9.0                                              # the padding row beats every other row
    lengths = torch.randint(0, 12, (B,), generator=gen)
    ids = _bag_ids(V, lengths, gen, lo=0)
    for b in range(0, B, 3):
        if ids[b].numel():
            ids[b][int(torch.randint(0, ids[b].numel(), (1,), generator=gen))] = P
    f = Feat("p", "T", ids, mask=P, junk=(2, 0))
    tables = {"T": (W, P)}
    dY = _dy(B, D, 4)
    out, argpos, grads = Dev([f], tables).run([f.bags()], dY)
    assert float(out.max()) < 9.0
    check("masked max", form(D) + " bags max masked", [f], tables, dY, out, argpos, grads)
    assert int(torch.count_nonzero(grads["T"][P])) == 0
    # padding_idx alone (no mask_id): the row is read in the forward and wins, and its gradient row stays zero
    from recbox_amd import ops
    p = torch.nn.Parameter(W.cuda())
    o = ops.embed_bags([ops.BagSpec("p", D, 0, 0, ops.POOL_MAX, V, padding_idx=P)], [f.bags()], [p])
    o.backward(dY.cuda())
    has = torch.tensor([bool((t == P).any()) for t in ids])
    assert bool((o.detach().cpu()[has] == 9.0).all()) and int(torch.count_nonzero(p.grad[P])) == 0


# ---- 5. the long form is bit-equal to the walk ---------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [64, 10, 260])
def test_long_form_is_bit_equal_to_the_walk_and_segment_zero_wins_a_tie(D):
    from recbox_amd import ops
    gen = torch.Generator().manual_seed(D)
    V = 500
    W = magnitudes((V, D), gen)
    W[V - 1] = 7.0                                          # the winner wherever it appears
    lengths = torch.tensor([0, 1, 255, 256, 257, 600] * 3 + [600])
    lengths = lengths[torch.randperm(lengths.numel(), generator=gen)]
    ids = _bag_ids(V - 1, lengths, gen, lo=0)
    tie = int((lengths == 600).nonzero()[0])
    ids[tie][10] = V - 1                                    # segment 0 ...
    ids[tie][300] = V - 1                                   # ... and segment 1 hold the same winning row
    f = Feat("l", "T", ids, junk=(7, 3))
    tables = {"T": (W, None)}
    dY = _dy(len(ids), D, 6)
    dev = Dev([f], tables)
    old = ops.bag_long_threshold(256)
    try:
        long_form = dev.run([f.bags()], dY)
        ops.bag_long_threshold(0)
        walk = dev.run([f.bags()], dY)
    finally:
        ops.bag_long_threshold(old)
    assert torch.equal(long_form[0], walk[0]) and torch.equal(long_form[1], walk[1])
    assert torch.equal(long_form[2]["T"], walk[2]["T"])
    assert bool((long_form[1][tie] == int(f.offsets[tie]) + 7 + 10).all())
    check("long max", form(D) + " bags max long", [f], tables, dY, *long_form)


# ---- 6. bad input goes through the status word -------------------------------------------------------------------------------
def test_out_of_range_ids_and_decreasing_offsets_raise_and_leave_the_well_formed_bags_correct():
    from recbox_amd import ops
    gen = torch.Generator().manual_seed(3)
    V, D, B = 300, 16, 200
    W = magnitudes((V, D), gen)
    lengths = torch.randint(0, 12, (B,), generator=gen)
    lengths[10:14] = torch.tensor([6, 5, 7, 4])
    lengths[50] = 5
    ids = _bag_ids(V, lengths, gen, lo=0)
    feats = [Feat(n, "T", ids) for n in ("good", "decreasing", "bad_id")]
    dev = Dev(feats, {"T": (W, None)})
    flat, offsets = feats[0].flat.cuda(), feats[0].offsets
    dec = offsets.clone()
    dec[12] = dec[11] - 3
    wrong = flat.clone()
    wrong[int(offsets[50])] = V
    clean = [ops.Bags(flat, offsets.cuda())] * 3
    with torch.no_grad():
        want = ops.embed_bags(dev.plan, clean, dev.plist()).cpu()
    old = ops.config.check_ids
    try:
        ops.config.check_ids = True
        for k, bad in ((1, ops.Bags(flat, dec.cuda())), (2, ops.Bags(wrong, offsets.cuda()))):
            call = list(clean)
            call[k] = bad
            with pytest.raises(IndexError):
                ops.embed_bags(dev.plan, call, dev.plist())
        ops.config.check_ids = False
        try:
            ops.check_deferred_ids()
        except IndexError:
            pass
        out = ops.embed_bags(dev.plan, [clean[0], ops.Bags(flat, dec.cuda()), ops.Bags(wrong, offsets.cuda())], dev.plist())
        out.backward(_dy(B, 3 * D, 9).cuda())               # sort + reduce clamp the same way: nothing faults
        with pytest.raises(IndexError):
            ops.check_deferred_ids()
    finally:
        ops.config.check_ids = old
    torch.cuda.synchronize()
    out = out.detach().cpu()
    assert torch.equal(out[:, :D], want[:, :D])
    intact = torch.ones(B, dtype=torch.bool)
    intact[11:13] = False
    assert torch.equal(out[intact, D:2 * D], want[intact, D:2 * D])
    assert int(torch.count_nonzero(out[11, D:2 * D])) == 0
    rest = torch.ones(B, dtype=torch.bool)
    rest[50] = False
    assert torch.equal(out[rest, 2 * D:], want[rest, 2 * D:])


# ---- 7. one captured step ------------------------------------------------------------------------------------------------------
def test_max_forward_loss_and_backward_captured_in_one_graph_replay_on_new_ids():
    from recbox_amd import ops
    gen = torch.Generator().manual_seed(8)
    V, D, B, nnz = 5000, 32, 513, 9000
    W = magnitudes((V, D), gen)

    def contents(seed):
        g = torch.Generator().manual_seed(seed)
        cuts = torch.sort(torch.randint(0, nnz + 1, (B - 1,), generator=g)).values
        return torch.randint(0, V, (nnz,), generator=g), torch.cat([torch.zeros(1, dtype=torch.int64), cuts, torch.tensor([nnz])])

    dev = Dev([Feat("s", "T", [])], {"T": (W, None)})
    table = dev.params["T"]
    scale = _dy(B, D, 3).cuda()
    idx0, off0 = contents(1)
    indices, offsets = idx0.cuda(), off0.to(torch.int32).cuda()
    bags = [ops.Bags(indices, offsets)]

    def step(b):
        out = ops.embed_bags(dev.plan, b, dev.plist())
        (out * scale).sum().backward()
        return out

    old = ops.config.check_ids
    try:
        ops.config.check_ids = False
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):                              # warm the plan up: workspaces of the replay
                table.grad = None
                step(bags)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        table.grad = None
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = step(bags)
        grad = table.grad
        for seed in (2, 3):
            idx1, off1 = contents(seed)
            indices.copy_(idx1.cuda())
            offsets.copy_(off1.to(torch.int32).cuda())
            graph.replay()
            torch.cuda.synchronize()
            got = out.detach().clone(), grad.clone()
            table.grad = None
            want = step([ops.Bags(idx1.cuda(), off1.cuda())])
            torch.cuda.synchronize()
            assert torch.equal(got[0], want.detach()) and torch.equal(got[1], table.grad)
            assert int(torch.count_nonzero(got[1])) > 0
            table.grad = grad
        ops.check_deferred_ids()
    finally:
        ops.config.check_ids = old


# ---- 8. persistent gradients and the sparse-row optimiser ------------------------------------------------------------------------
def test_three_steps_over_the_gradient_pool_with_sparse_sgd_against_dense_sgd_in_float64():
    """reuse_grad_buffers = "all": the pool, rbx_embed_csr_rezero between the steps, the TouchedRows record of kind "bags" and
    rbx_embed_csr_sparse_update.  Reference: torch.optim.SGD on a float64 copy through torch's CPU max.  Bound: a step adds
    lr * (gradient error <= C_BOUND eps32 A_k) and one rounding of the updated entry (<= eps32 |p|), so after the steps
    |p - ref| <= C_BOUND eps32 * sum_k (lr A_k + |ref_k|) -- the project's bound with that A."""
    from recbox_amd import ops, optim
    gen = torch.Generator().manual_seed(21)
    V, D, lr = 400, 20, 0.05
    W = magnitudes((V, D), gen)
    dev = Dev([Feat("s", "T", [])], {"T": (W, None)})
    table = dev.params["T"]
    opt = optim.SparseSGD([table], lr=lr)
    ref = W.double().clone().requires_grad_(True)
    ref_opt = torch.optim.SGD([ref], lr=lr)
    A = torch.zeros(V, D, dtype=torch.float64)
    old = ops.config.reuse_grad_buffers
    try:
        ops.config.reuse_grad_buffers = "all"
        for k, B in enumerate([150, 333, 64]):
            lengths = torch.randint(0, 15, (B,), generator=gen)
            f = Feat("s", "T", _bag_ids(V, lengths, gen, lo=0))
            dY = _dy(B, D, 30 + k)
            opt.zero_grad()
            ops.embed_bags(dev.plan, [f.bags()], dev.plist()).backward(dY.cuda())
            opt.step()
            ref_opt.zero_grad()
            out = cpu_max(f.flat, ref, f.offsets)
            (a,) = torch.autograd.grad(out, ref, dY.double().abs(), retain_graph=True)
            out.backward(dY.double())
            ref_opt.step()
            A += lr * a + ref.detach().abs()
            torch.cuda.synchronize()
            r = bound_ratio(table.detach(), ref.detach(), A)
            print("max pool + SparseSGD step %d: err / bound %.3g" % (k, r))
            assert r <= 1.0, "step %d: %.3g x the bound" % (k, r)
        assert opt.calls["dense"] == 0 and opt.calls["rows"] == 3, opt.calls
    finally:
        ops.config.reuse_grad_buffers = old
        ops.config.track_touched_rows = False


# ---- 9. shared and frozen tables ----------------------------------------------------------------------------------------------
def test_table_shared_by_a_max_call_and_a_sum_call_and_a_frozen_table():
    from recbox_amd import ops
    gen = torch.Generator().manual_seed(13)
    V, D, B = 300, 24, 170
    W = magnitudes((V, D), gen)
    fa = Feat("peak", "T", _bag_ids(V, torch.randint(0, 20, (B,), generator=gen), gen, lo=0))
    fb = Feat("total", "T", _bag_ids(V, torch.randint(0, 20, (B,), generator=gen), gen, lo=0))
    dYa, dYb = _dy(B, D, 1), _dy(B, D, 2)
    p = torch.nn.Parameter(W.cuda())
    omax = ops.embed_bags([ops.BagSpec("peak", D, 0, 0, ops.POOL_MAX, V)], [fa.bags()], [p])
    osum = ops.embed_bags([ops.BagSpec("total", D, 0, 0, ops.POOL_SUM, V)], [fb.bags()], [p])
    ((omax * dYa.cuda()).sum() + (osum * dYb.cuda()).sum()).backward()
    torch.cuda.synchronize()
    leaf = W.double().clone().requires_grad_(True)
    rmax = cpu_max(fa.flat, leaf, fa.offsets)
    rsum = F.embedding_bag(fb.flat, leaf, fb.offsets, mode="sum", include_last_offset=True)
    both = (rmax * dYa.double()).sum() + (rsum * dYb.double()).sum()
    (g,) = torch.autograd.grad(both, leaf, retain_graph=True)
    (a,) = torch.autograd.grad((rmax * dYa.double().abs()).sum() + (rsum * dYb.double().abs()).sum(), leaf)
    assert torch.equal(omax.detach().cpu(), cpu_max(fa.flat, W, fa.offsets))
    r = bound_ratio(p.grad, g, a)
    assert r <= 1.0 and int(torch.count_nonzero(p.grad.cpu()[a == 0])) == 0, r
    # frozen: no sort, no gradient, the same forward
    frozen = torch.nn.Parameter(W.cuda(), requires_grad=False)
    scale = torch.ones(B, D, device="cuda", requires_grad=True)
    o = ops.embed_bags([ops.BagSpec("peak", D, 0, 0, ops.POOL_MAX, V)], [fa.bags()], [frozen])
    assert o.grad_fn is None and torch.equal(o.cpu(), omax.detach().cpu())
    (o * scale).sum().backward()
    assert frozen.grad is None


# ---- 10. refusals through ops ---------------------------------------------------------------------------------------------------
def test_refusals_weights_on_max_mixed_plans_and_max_in_a_padded_field():
    from recbox_amd import ops
    idx, off = torch.tensor([1, 2, 3]).cuda(), torch.tensor([0, 1, 3]).cuda()
    p = torch.nn.Parameter(torch.zeros(5, 4).cuda())
    with pytest.raises(NotImplementedError, match="per.sample weights"):
        ops.embed_bags([ops.BagSpec("m", 4, 0, 0, ops.POOL_MAX, 5)], [ops.Bags(idx, off, torch.ones(3).cuda())], [p])
    with pytest.raises(NotImplementedError, match="call of their own"):
        ops.embed_bags([ops.BagSpec("m", 4, 0, 0, ops.POOL_MAX, 5), ops.BagSpec("s", 4, 4, 0, ops.POOL_SUM, 5)],
                       [ops.Bags(idx, off)] * 2, [p])
    spec = ops.FieldSpec("h", 0, 4, 0, param=0, pool=ops.POOL_MAX, seq_len=3, vocab=5)
    with pytest.raises((ValueError, NotImplementedError)):
        ops.embed_lookup(ops.EmbedPlan([spec], 4), [torch.zeros(2, 3, dtype=torch.long).cuda()], [p])


# ---- 11. the nn.Module ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["sum", "mean", "max"])
@pytest.mark.parametrize("last", [False, True])
def test_embedding_bag_module_against_torch_nn_embedding_bag_on_the_cpu(mode, last):
    """1-D input with offsets (with and without include_last_offset; an empty bag in the middle and, without the last offset,
    at the end), 2-D input, padding_idx set, per_sample_weights for sum.  Forward: max exact, sum / mean at
    max(C_BOUND, Lmax + 2) eps32 A with A the same pool over |W|; weight gradient at C_BOUND eps32 A."""
    from recbox_amd.bag import EmbeddingBag
    gen = torch.Generator().manual_seed(17)
    V, D, B, P = 60, 12, 50, 4
    W = magnitudes((V, D), gen)
    lengths = torch.randint(0, 9, (B,), generator=gen)
    lengths[5] = 0
    lengths[B - 1] = 0 if not last else 3
    flat = torch.cat(_bag_ids(V, lengths, gen, lo=0))
    offsets = torch.zeros(B + 1, dtype=torch.int64)
    torch.cumsum(lengths, 0, out=offsets[1:])
    offs = offsets if last else offsets[:-1]
    two_d = torch.randint(0, V, (B, 6), generator=gen)
    cases = [(flat, offs, None), (two_d, None, None)]
    if mode == "sum":
        cases += [(flat, offs, magnitudes((flat.numel(),), gen)), (two_d, None, magnitudes((B, 6), gen))]
    dY = _dy(B, D, 19)
    Lmax = int(max(lengths.max(), 6))
    for pad in (None, P):
        dut = EmbeddingBag(V, D, mode=mode, padding_idx=pad, include_last_offset=last, _weight=W.clone()).cuda()
        for inp, off, psw in cases:
            def run(module, dy, dev, w=psw):
                module.weight.grad = None
                args = [t.to(dev) if t is not None else None for t in (inp, off)]
                out = module(args[0], args[1], per_sample_weights=w.to(dev).to(module.weight.dtype) if w is not None else None)
                out.backward(dy.to(dev).to(out.dtype))
                return out.detach().cpu(), module.weight.grad.detach().cpu()

            ref = torch.nn.EmbeddingBag(V, D, mode=mode, padding_idx=pad, include_last_offset=last, _weight=W.double().clone())
            want, gwant = run(ref, dY, "cpu")
            if mode == "max":
                a_out, (_, ga) = None, run(ref, dY.abs(), "cpu")
            else:
                aref = torch.nn.EmbeddingBag(V, D, mode=mode, padding_idx=pad, include_last_offset=last,
                                             _weight=W.double().abs().clone())
                a_out, ga = run(aref, dY.abs(), "cpu", psw.abs() if psw is not None else None)
            out, g = run(dut, dY, "cuda")
            torch.cuda.synchronize()
            tag = "%s last=%s pad=%s %s%s" % (mode, last, pad, "2-D" if off is None else "1-D", " weighted" if psw is not None else "")
            if mode == "max":
                ref32 = torch.nn.EmbeddingBag(V, D, mode=mode, padding_idx=pad, include_last_offset=last, _weight=W.clone())
                assert torch.equal(out, ref32(inp, off).detach()), tag
            else:
                r = bound_ratio(out, want, a_out, max(C_BOUND, Lmax + 2))
                assert r <= 1.0, "%s: forward %.3g x the bound" % (tag, r)
            if off is not None:
                assert int(torch.count_nonzero(out[5])) == 0, "%s: the empty bag is not a zero row" % tag
                if not last:
                    assert int(torch.count_nonzero(out[B - 1])) == 0, tag
            if pad is not None:
                ga[pad] = 0
                gwant[pad] = 0
            r = bound_ratio(g, gwant, ga)
            assert r <= 1.0 and int(torch.count_nonzero(g[ga == 0])) == 0, "%s: weight gradient %.3g x the bound" % (tag, r)


def test_embedding_bag_mean_eps_leaves_non_empty_bags_bit_equal_to_eps_zero():
    from recbox_amd import ops
    from recbox_amd.bag import MEAN_EPS, EmbeddingBag
    gen = torch.Generator().manual_seed(23)
    V, D, B = 80, 16, 64
    W = magnitudes((V, D), gen)
    lengths = torch.randint(1, 40, (B,), generator=gen)
    f = Feat("m", "T", _bag_ids(V, lengths, gen, lo=0))
    m = EmbeddingBag(V, D, mode="mean", include_last_offset=True, _weight=W.clone()).cuda()
    with torch.no_grad():
        got = m(f.flat.cuda(), f.offsets.cuda())
        zero = ops.embed_bags([ops.BagSpec("m", D, 0, 0, ops.POOL_MEAN_ID, V, eps=0.0)], [f.bags()], [m.weight])
    assert MEAN_EPS == 2.0 ** -126 and torch.equal(got, zero)
