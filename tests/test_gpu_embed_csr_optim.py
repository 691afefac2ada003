"""Training a table through the ragged (CSR) lookup: rbx_embed_csr_sparse_update / rbx_embed_csr_rezero on the C ABI,
``ops.embed_bags`` over the persistent gradient pool (``ops.config.reuse_grad_buffers = "all"``), and
recbox_amd.optim's sparse-row optimisers over the "bags" record of touched rows -- eagerly and captured into one graph.

Reference: ``_reference_step`` of tests/test_gpu_optim.py (the sparse branches of torch.optim in plain torch) applied to
the rows the batch looked up, computed here from ``indices`` / ``offsets`` with torch ops.  Tolerances are that file's:
tables atol 2e-6, optimiser state atol 1e-6; every row the batch did not look up must be bit-identical."""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import _note  # noqa: E402
from test_gpu_optim import _make, _reference_step  # noqa: E402

TABLE_ATOL, STATE_ATOL = 2e-6, 1e-6
HP = {"sgd": {"lr": 0.05}, "adagrad": {"lr": 0.05, "eps": 1e-10}, "adam": {"lr": 0.01, "betas": (0.9, 0.999), "eps": 1e-8}}
FROZEN_STATE = 123.0


def _close(what, got, want, atol):
    err = float((got - want).abs().max()) if got.numel() else 0.0
    _note(what, err, atol)
    assert err <= atol, "%s: %.3e > %.1e" % (what, err, atol)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ragged(V, B, gen, lo=0, zipf=False, head=3, tail=5, lmax=12, avoid=(), outside=None):
    """indices / offsets (CPU, int64) of B bags: ``head`` ids in front of the first bag and ``tail`` behind the last one,
    bag B // 2 empty, ids in [lo, V) without ``avoid``; ``outside``: the id the positions outside every bag hold (and no
    position inside one)."""
    lengths = torch.randint(0, lmax, (B,), generator=gen)
    lengths[B // 2] = 0
    lengths[0] = max(int(lengths[0]), 2)
    nnz = head + int(lengths.sum()) + tail
    u = torch.rand(nnz, generator=gen)
    ids = (lo + ((V - lo) * (u ** 3 if zipf else u)).long()).clamp_(max=V - 1)
    banned = list(avoid) + ([outside] if outside is not None else [])
    spare = [i for i in range(lo, V) if i not in banned][0]
    for a in banned:
        ids[ids == a] = spare
    if outside is not None:
        ids[:head] = outside
        ids[nnz - tail:] = outside
    offsets = head + torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(lengths, 0)])
    return ids, offsets


def _looked_up(ids, offsets, V, pad=None, mask=None):
    """The rows a bag descriptor touches: ids inside a bag, in range, neither padding_idx nor (``mask``) the masked id."""
    live = ids[int(offsets[0]):int(offsets[-1])]
    live = live[(live >= 0) & (live < V)]
    if pad is not None:
        live = live[live != pad]
    if mask is not None:
        live = live[live != mask]
    return torch.unique(live)


class Call(object):
    """One C-ABI call over a frozen descriptor (slot 0) and trained ones behind it: tables, gradients, state, the
    descriptors' batch, and the rows each table must see stepped."""

    def __init__(self, rule, dims, B=257, seed=0, weighted=False):
        from recbox_amd import _lib, ops
        self.rule, self.B, self.weighted = rule, B, weighted
        gen = torch.Generator().manual_seed(1000 + seed)
        dA, dB, dC = dims
        S, MI, SI = _lib.POOL_SUM, _lib.POOL_MEAN_ID, _lib.POOL_SUM_ID
        # (name, table, vocab, dim, pool, padding_idx, mask_id, eps): table "B" is read by two descriptors
        feats = [("frozen", "F", 11, dA, S, None, None, 0.0),
                 ("a", "A", 5, dA, S, 0, None, 0.0),
                 ("b_mean", "B", 3001, dB, S if weighted else MI, 0, None if weighted else 7, 1e-3),
                 ("c", "C", 70000, dC, SI, 1, 9, 0.0),
                 ("b_sum", "B", 3001, dB, S, 0, None, 0.0)]
        self.names, self.vocab, self.dim = ["F", "A", "B", "C"], {}, {}
        specs, tensors, off = [], [], 0
        self.rows = dict((t, []) for t in self.names)
        self.never = dict((t, []) for t in self.names)          # rows named in the batch that must NOT be stepped
        for name, tab, V, D, pool, pad, mask, eps in feats:
            self.vocab[tab], self.dim[tab] = V, D
            outside = V - 1
            avoid = [7] if tab == "B" else []                   # b_sum never names the row b_mean masks
            ids, offsets = _ragged(V, B, gen, zipf=(name in ("c", "b_sum")), avoid=avoid, outside=outside)
            at = int(offsets[0])
            if pad is not None:
                ids[at] = pad                                   # a padding_idx id inside the first bag
            if mask is not None:
                ids[at + 1] = mask                              # ... and a mask_id id
            if name == "c":
                ids[int(offsets[-1]) - 1] = V + 13              # one id outside [0, vocab): flagged, never looked up
            specs.append(ops.BagSpec(name, D, off, self.names.index(tab), pool, V, padding_idx=pad, mask_id=mask, eps=eps))
            off += D
            dtype = torch.int32 if name == "a" else torch.int64
            tensors += [ids.to(dtype).cuda(), offsets.to(dtype).cuda()]
            id_pool = pool in (MI, SI)
            if tab != "F":
                self.rows[tab].append(_looked_up(ids, offsets, V, pad, mask if id_pool else None))
                self.never[tab] += [outside] + ([pad] if pad is not None else []) + ([mask] if id_pool and mask is not None else [])
            assert int(offsets[B // 2 + 1]) == int(offsets[B // 2]) and int(offsets[0]) > 0 and int(offsets[-1]) < ids.numel()
        self.rows = dict((t, torch.unique(torch.cat(r)).cuda() if r else None) for t, r in self.rows.items())
        self.width = off
        self.plan, self.tensors = ops.BagPlan(specs, off), tensors
        self.tables = [torch.randn(self.vocab[t], self.dim[t], generator=gen).mul_(0.1).cuda() for t in self.names]
        self.grads = [None] + [torch.zeros_like(t) for t in self.tables[1:]]
        # state away from zero, so that an untouched row that was read or written shows; second moments >= 0.5: the step
        # stays of the size the tolerances were set for (1 / sqrt(v) of a v near zero would magnify one ulp of v)
        self.s1 = [torch.rand(t.shape, generator=gen).mul_(0.5).add_(0.25).cuda() for t in self.tables]
        self.s2 = [torch.rand(t.shape, generator=gen).add_(0.5).cuda() for t in self.tables]
        self.s1[0].fill_(FROZEN_STATE)
        self.s2[0].fill_(FROZEN_STATE)
        self.weights = None
        if weighted:
            self.weights = [torch.rand(tensors[2 * k].numel(), generator=gen).add_(0.5).cuda() for k in range(len(feats))]
        # the upstream gradient of a batch-mean loss (the scale tests/test_gpu_optim.py's absolute tolerances belong to:
        # a hot row's Adagrad sum stays below 1, where one ulp is 6e-8)
        self.dY = torch.randn(B, off, generator=gen).div_(B).cuda()
        self.status = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.ws = None

    def _state_arrays(self, s1, s2):
        n_state = {"sgd": 0, "adagrad": 1, "adam": 2}[self.rule]
        out = []
        for k, src in enumerate((s1, s2)):
            arr = (ctypes.c_void_p * self.plan.n)()
            for i, sp in enumerate(self.plan.specs):            # by DESCRIPTOR index; shared tables pass the same pointer
                arr[i] = src[sp.param].data_ptr() if k < n_state else None
            out.append(arr if k < n_state else None)
        return out

    def sort_and_backward(self):
        from recbox_amd._lib import check, lib
        plan, B = self.plan, self.B
        plan.bind_tensors(self.tensors)
        plan.bind_params(self.tables, self.grads)
        ws_bytes = lib.rbx_embed_csr_bwd_workspace_size(plan.arr, plan.n, B)
        assert ws_bytes > 0
        self.ws, self.ws_bytes = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda"), ws_bytes
        if self.weighted:
            warr = (ctypes.c_void_p * plan.n)(*[w.data_ptr() for w in self.weights])
            check(lib.rbx_embed_csr_sort_weighted(plan.arr, plan.n, B, _ptr(self.ws), ws_bytes, _ptr(self.status), _stream()))
            check(lib.rbx_embed_csr_bwd_weighted(plan.arr, plan.n, B, warr, _ptr(self.dY), self.width, 0, _ptr(self.ws), ws_bytes,
                                                 _stream()))
        else:
            out = torch.empty(B, self.width, device="cuda")
            scale = torch.empty(plan.n, B, device="cuda")
            check(lib.rbx_embed_csr_fwd(plan.arr, plan.n, B, _ptr(out), self.width, _ptr(scale), None, _stream()))
            check(lib.rbx_embed_csr_sort(plan.arr, plan.n, B, _ptr(self.ws), ws_bytes, _ptr(self.status), _stream()))
            check(lib.rbx_embed_csr_bwd(plan.arr, plan.n, B, _ptr(self.dY), self.width, _ptr(scale), 0, _ptr(self.ws), ws_bytes,
                                        _stream()))
        torch.cuda.synchronize()
        assert int(self.status.item()) & 1, "the out-of-range id was not flagged"

    def update(self, tables, grads, s1, s2, clear=0):
        from recbox_amd import _lib
        from recbox_amd._lib import check, lib
        hp = HP[self.rule]
        lr = hp["lr"]
        b1, b2 = hp.get("betas", (0.0, 0.0))
        if self.rule == "adam":
            lr = lr * math.sqrt(1 - b2) / (1 - b1)              # step 1, folded in by the caller
        kind = {"sgd": _lib.OPT_SGD, "adagrad": _lib.OPT_ADAGRAD, "adam": _lib.OPT_ADAM}[self.rule]
        opt = _lib.rbx_opt_t(kind, lr, b1, b2, hp.get("eps", 0.0), 0.0, None)
        self.plan.bind_tensors(self.tensors)
        self.plan.bind_params(tables, grads)
        a1, a2 = self._state_arrays(s1, s2)
        check(lib.rbx_embed_csr_sparse_update(self.plan.arr, self.plan.n, self.B, _ptr(self.ws), self.ws_bytes, ctypes.byref(opt),
                                              a1, a2, clear, _stream()))
        torch.cuda.synchronize()

    def check_step(self, tag, tables, s1, s2):
        """tables / state after ONE step from self.tables / self.s1 / self.s2 with self.grads."""
        rule = self.rule
        assert torch.equal(tables[0], self.tables[0]), "the frozen table moved"
        assert bool((s1[0] == FROZEN_STATE).all()) and bool((s2[0] == FROZEN_STATE).all()), "the frozen slot's state was written"
        for k in range(1, len(self.names)):
            name, rows = self.names[k], self.rows[self.names[k]]
            ref = self.tables[k].clone()
            st = {"step": 0, "sum": self.s1[k].clone(), "m": self.s1[k].clone(), "v": self.s2[k].clone()}
            touched_by_grad = (self.grads[k] != 0).any(dim=1).nonzero().reshape(-1)
            assert bool(torch.isin(touched_by_grad, rows).all()), "%s: the backward wrote a row the batch does not name" % name
            assert rows.numel() > 0
            _reference_step(rule, ref, self.grads[k], rows, st, HP[rule])
            _close("%s table %s" % (tag, name), tables[k], ref, TABLE_ATOL)
            mask = torch.zeros(tables[k].shape[0], dtype=torch.bool, device="cuda")
            mask[rows] = True
            assert torch.equal(tables[k][~mask], self.tables[k][~mask]), "%s: an untouched row of table %s changed" % (tag, name)
            assert not torch.equal(tables[k][mask], self.tables[k][mask])
            for r in self.never[name]:                           # padding_idx, mask_id, the id outside every bag: by name
                assert not bool(mask[r]) and torch.equal(tables[k][r], self.tables[k][r]), (tag, name, r)
                assert torch.equal(s1[k][r], self.s1[k][r]) and torch.equal(s2[k][r], self.s2[k][r]), (tag, name, r)
            if rule == "sgd":
                assert torch.equal(s1[k], self.s1[k]) and torch.equal(s2[k], self.s2[k])
                continue
            _close("%s state1 %s" % (tag, name), s1[k], st["sum"] if rule == "adagrad" else st["m"], STATE_ATOL)
            assert torch.equal(s1[k][~mask], self.s1[k][~mask]), "%s: untouched state of %s changed" % (tag, name)
            if rule == "adam":
                _close("%s state2 %s" % (tag, name), s2[k], st["v"], STATE_ATOL)
                assert torch.equal(s2[k][~mask], self.s2[k][~mask])
            else:
                assert torch.equal(s2[k], self.s2[k])


def _clones(ts):
    return [t.clone() if t is not None else None for t in ts]


# dim 1 / 10 scalar, 16 / 128 float4, 260 float4 with 65 lane units and 67 scalar (the stride loop runs twice), mixed
DIMS = [(1, 1, 1), (10, 10, 10), (16, 16, 16), (128, 128, 128), (260, 260, 260), (67, 67, 67), (16, 10, 16)]


@pytest.mark.parametrize("dims", DIMS, ids=lambda d: "x".join(map(str, d)))
@pytest.mark.parametrize("rule", ["sgd", "adagrad", "adam"])
def test_c_abi_steps_exactly_the_looked_up_rows(rule, dims):
    """sort -> backward -> update over a frozen descriptor in front of four trained ones (two share a table, one mean pool
    with eps > 0, int32 and int64 ids): looked-up rows equal the torch rule, every other row of tables and state is
    bit-identical -- the padding_idx row, the mask_id row, the id outside every bag and the empty bag among them.  Then
    clear_grad = 1 from the same start: every gradient all-zero, tables and state bit-equal to clear_grad = 0."""
    c = Call(rule, dims, seed=sum(dims))
    c.sort_and_backward()
    t0, a0, b0 = _clones(c.tables), _clones(c.s1), _clones(c.s2)
    g0 = _clones(c.grads)
    c.update(t0, g0, a0, b0, clear=0)
    c.check_step("%s %s" % (rule, dims), t0, a0, b0)
    for g, want in zip(g0[1:], c.grads[1:]):
        assert torch.equal(g, want), "clear_grad = 0 wrote a gradient"
    t1, a1, b1 = _clones(c.tables), _clones(c.s1), _clones(c.s2)
    g1 = _clones(c.grads)
    c.update(t1, g1, a1, b1, clear=1)
    for g in g1[1:]:
        assert int(torch.count_nonzero(g)) == 0, "clear_grad = 1 left gradient rows behind"
    for got, want in zip(t1 + a1 + b1, t0 + a0 + b0):
        assert torch.equal(got, want), "clear_grad = 1 changed the step"


@pytest.mark.parametrize("dims", [(16, 16, 16), (10, 10, 10)], ids=["vec", "scalar"])
@pytest.mark.parametrize("rule", ["sgd", "adam"])
def test_c_abi_weighted_sort_is_stepped_through_the_same_entry_point(rule, dims):
    c = Call(rule, dims, seed=5, weighted=True)
    c.sort_and_backward()
    t0, a0, b0, g0 = _clones(c.tables), _clones(c.s1), _clones(c.s2), _clones(c.grads)
    c.update(t0, g0, a0, b0, clear=0)
    c.check_step("weighted %s %s" % (rule, dims), t0, a0, b0)
    t1, a1, b1, g1 = _clones(c.tables), _clones(c.s1), _clones(c.s2), _clones(c.grads)
    c.update(t1, g1, a1, b1, clear=1)
    assert all(int(torch.count_nonzero(g)) == 0 for g in g1[1:])
    assert all(torch.equal(x, y) for x, y in zip(t1 + a1 + b1, t0 + a0 + b0))


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("dims", [(16, 16, 16), (16, 10, 16), (260, 260, 260)], ids=["vec", "mixed", "wide"])
def test_c_abi_rezero_clears_the_stored_rows_and_nothing_else(dims, weighted):
    from recbox_amd._lib import check, lib
    c = Call("sgd", dims, seed=9, weighted=weighted)
    c.sort_and_backward()
    masks = []
    for k in range(1, len(c.names)):
        mask = torch.zeros(c.tables[k].shape[0], dtype=torch.bool, device="cuda")
        mask[c.rows[c.names[k]]] = True
        assert int(torch.count_nonzero(c.grads[k][mask])) > 0
        c.grads[k][~mask] = 7.0
        masks.append(mask)
    c.plan.bind_tensors(c.tensors)
    c.plan.bind_params(c.tables, c.grads)
    check(lib.rbx_embed_csr_rezero(c.plan.arr, c.plan.n, c.B, _ptr(c.ws), c.ws_bytes, _stream()))
    torch.cuda.synchronize()
    for k, mask in zip(range(1, len(c.names)), masks):
        assert int(torch.count_nonzero(c.grads[k][mask])) == 0, "a stored row of %s was not cleared" % c.names[k]
        assert bool((c.grads[k][~mask] == 7.0).all()), "a row of %s nobody stored was written" % c.names[k]


# ---- ops.embed_bags over the persistent gradients -----------------------------------------------------------------------
def _bag_model(seed=3):
    """Two plans as a model would hold them: three unweighted features (mixed pools, two of them on one table) and one
    weighted feature with a table of its own."""
    from recbox_amd import _lib, ops
    gen = torch.Generator().manual_seed(seed)
    D = 16
    tables = [torch.nn.Parameter(torch.randn(V, D, generator=gen).mul_(0.1).cuda()) for V in (3001, 70000, 503)]
    plan = ops.BagPlan([ops.BagSpec("m", D, 0, 0, _lib.POOL_MEAN_ID, 3001, padding_idx=0, mask_id=0, eps=1e-8),
                        ops.BagSpec("s", D, D, 1, _lib.POOL_SUM_ID, 70000, padding_idx=0, mask_id=0),
                        ops.BagSpec("t", D, 2 * D, 0, _lib.POOL_SUM, 3001, padding_idx=0)])
    wplan = ops.BagPlan([ops.BagSpec("w", D, 0, 0, _lib.POOL_SUM, 503, padding_idx=0)])
    return tables, plan, wplan


def _bag_batch(B, seed):
    from recbox_amd import ops
    gen = torch.Generator().manual_seed(seed)
    bags = []
    for k, V in enumerate((3001, 70000, 3001, 503)):
        ids, offsets = _ragged(V, B, gen, zipf=bool((k + seed) % 2))
        w = torch.rand(ids.numel(), generator=gen).add_(0.5).cuda() if k == 3 else None
        bags.append(ops.Bags(ids.cuda(), offsets.cuda(), w))
    dY = torch.randn(B, 48, generator=gen).div_(B).cuda()
    dYw = torch.randn(B, 16, generator=gen).div_(B).cuda()
    return bags, dY, dYw


def _bag_step(tables, plan, wplan, batch):
    from recbox_amd import ops
    bags, dY, dYw = batch
    for p in tables:
        p.grad = None
    out = ops.embed_bags(plan, bags[:3], tables[:2])
    outw = ops.embed_bags(wplan, bags[3:], tables[2:])
    torch.autograd.backward([out, outw], [dY, dYw])
    torch.cuda.synchronize()


def _in(buf, t):
    return buf is not None and buf.data_ptr() <= t.data_ptr() < buf.data_ptr() + buf.numel() * 4


def test_embed_bags_over_the_gradient_pool_gives_the_bits_of_fresh_gradients():
    """B = 300, 700, 64, 700 (the workspace grows, a smaller batch, the old size again): p.grad is bit-equal to the step
    with the setting off, it aliases the pool's buffer, and the buffer holds nothing but this step's rows."""
    from recbox_amd import ops
    tables, plan, wplan = _bag_model()
    old = ops.config.reuse_grad_buffers
    try:
        for k, B in enumerate([300, 700, 64, 700]):
            batch = _bag_batch(B, 20 + k)
            ops.config.reuse_grad_buffers = False
            _bag_step(tables, plan, wplan, batch)
            want = [p.grad.clone() for p in tables]
            assert not hasattr(plan, "_grad_pools") or not any(_in(pl.flat, tables[0].grad) for pl in plan._grad_pools.values())
            ops.config.reuse_grad_buffers = "all"
            _bag_step(tables, plan, wplan, batch)
            pool, wpool = plan._grad_pools[False], wplan._grad_pools[True]
            for p, w, owner in zip(tables, want, (pool, pool, wpool)):
                assert torch.equal(p.grad, w), "step %d: pooled gradient differs from the fresh one" % k
                assert _in(owner.flat, p.grad), "step %d: p.grad does not alias the persistent buffer" % k
            assert pool.dirty_batch == B and wpool.dirty_batch == B
            bags = batch[0]
            for p, feats in ((tables[0], (bags[0], bags[2])), (tables[1], (bags[1],)), (tables[2], (bags[3],))):
                mask = torch.zeros(p.shape[0], dtype=torch.bool, device="cuda")
                for g in feats:
                    mask[g.indices[int(g.offsets[0]):int(g.offsets[-1])]] = True
                assert int(torch.count_nonzero(p.grad[~mask])) == 0, "step %d: rows of an earlier step are still there" % k
                assert int(torch.count_nonzero(p.grad[mask])) > 0
        # two training forwards before one backward: both get fresh gradients, the buffer stays as it is
        batch = _bag_batch(300, 31)
        for p in tables:
            p.grad = None
        o1 = ops.embed_bags(plan, batch[0][:3], tables[:2])
        o2 = ops.embed_bags(plan, batch[0][:3], tables[:2])
        torch.autograd.backward([o1, o2], [batch[1], batch[1]])
        torch.cuda.synchronize()
        assert not _in(plan._grad_pools[False].flat, tables[0].grad) and not _in(plan._grad_pools[False].flat, tables[1].grad)
        ops.config.reuse_grad_buffers = False
        two = [tables[0].grad.clone(), tables[1].grad.clone()]
        _bag_step(tables, plan, wplan, batch)
        for got, p in zip(two, tables[:2]):
            _close("two forwards, one backward", got, 2 * p.grad, 1e-5 * float(p.grad.abs().max()))
        # a backward that finds p.grad set: the RuntimeError of the generic lookup
        ops.config.reuse_grad_buffers = "all"
        _bag_step(tables, plan, wplan, batch)
        out = ops.embed_bags(plan, batch[0][:3], tables[:2])           # (p.grad still holds the last step's gradient)
        with pytest.raises(RuntimeError, match=r"zero_grad\(set_to_none=True\)"):
            out.backward(batch[1])
    finally:
        ops.config.reuse_grad_buffers = old
        torch.cuda.synchronize()


# ---- the optimisers end to end ----------------------------------------------------------------------------------------------
def _layer(shared=False):
    from recbox_amd.rechub.basic.features import SequenceFeature, SparseFeature
    from recbox_amd.rechub.basic.layers import EmbeddingLayer
    D = 16
    if shared:
        feats = [SparseFeature("b", 300, D), SequenceFeature("hist_b", 300, D, pooling="mean", shared_with="b", padding_idx=0)]
    else:
        feats = [SequenceFeature("hist_c", 3001, D, pooling="sum", padding_idx=0),
                 SequenceFeature("hist_d", 70000, D, pooling="mean", padding_idx=0),
                 SequenceFeature("hist_w", 503, D, pooling="sum", padding_idx=0)]
    layer = EmbeddingLayer(feats).cuda()
    gen = torch.Generator().manual_seed(17)
    with torch.no_grad():
        for p in layer.parameters():
            p.copy_(torch.randn(p.shape, generator=gen).mul_(0.2))
    return layer, feats


def _layer_batch(B, seed):
    """x for _layer(): hist_c / hist_d unweighted Bags, hist_w weighted; the rows each table has looked up (id 0 is both
    padding_idx and the mask id of rechub's pools)."""
    from recbox_amd import ops
    gen = torch.Generator().manual_seed(seed)
    x, rows = {}, {}
    for k, (name, V) in enumerate((("hist_c", 3001), ("hist_d", 70000), ("hist_w", 503))):
        ids, offsets = _ragged(V, B, gen, zipf=bool((k + seed) % 2))
        w = torch.rand(ids.numel(), generator=gen).add_(0.5).cuda() if name == "hist_w" else None
        x[name] = ops.Bags(ids.cuda(), offsets.cuda(), w)
        rows[name] = _looked_up(ids, offsets, V, pad=0).cuda()
    return x, rows, torch.randn(B, 48, generator=gen).div_(B).cuda()      # (a batch-mean loss's upstream gradient)


def _pools_of(layer):
    """The gradient pools of the layer's bag plans (EmbeddingLayer caches (plan, bag plans, ...) per feature set)."""
    pools = []
    for key, cached in layer._plans.items():
        if isinstance(key, tuple) and key and key[0] == "bags":
            for bp in cached[1]:
                if bp is not None:
                    pools += list(getattr(bp, "_grad_pools", {}).values())
    return pools


@pytest.mark.parametrize("clear", [False, True], ids=["rezero", "clear_grads"])
@pytest.mark.parametrize("rule", ["sgd", "adagrad", "adam"])
def test_sparse_optimisers_step_a_bag_fed_layer_through_its_sorted_ids(rule, clear):
    """rechub's EmbeddingLayer fed ops.Bags (one unweighted embed_bags call, one weighted): three steps with fresh gradients,
    then three over the persistent pool.  Every table equals the torch rule on the looked-up rows at every step; no dense
    fallback, no union, one sparse-row call per embed_bags call.  clear_grads: the pool is clean after every step."""
    from recbox_amd import ops
    layer, feats = _layer()
    tables = dict((f.name, layer.embed_dict[f.name].weight) for f in feats)
    opt, hp = _make(rule, list(tables.values()))
    opt.clear_grads = clear
    ref = dict((n, p.detach().clone()) for n, p in tables.items())
    init = dict((n, p.detach().clone()) for n, p in tables.items())
    state = dict((n, {"step": 0, "sum": torch.zeros_like(p), "m": torch.zeros_like(p), "v": torch.zeros_like(p)})
                 for n, p in tables.items())
    ever = dict((n, torch.zeros(p.shape[0], dtype=torch.bool, device="cuda")) for n, p in tables.items())
    old = ops.config.reuse_grad_buffers
    calls = 0
    try:
        for flag in (False, "all"):
            ops.config.reuse_grad_buffers = flag
            for k, B in enumerate([300, 700, 64]):
                x, rows, dY = _layer_batch(B, 50 + k + 10 * int(bool(flag)))
                opt.zero_grad()
                layer(x, feats, squeeze_dim=True).backward(dY)
                grads = dict((n, p.grad.detach().clone()) for n, p in tables.items())
                opt.step()
                calls += 2
                pools = _pools_of(layer)
                for n, p in tables.items():
                    ever[n][rows[n]] = True
                    _reference_step(rule, ref[n], grads[n], rows[n], state[n], hp)
                    _close("%s %s step %d pool=%s" % (rule, n, k, flag), p.detach(), ref[n], TABLE_ATOL)
                    if flag and clear:
                        assert int(torch.count_nonzero(p.grad)) == 0, "clear_grads left rows of %s behind" % n
                if flag:
                    assert len(pools) == 2
                    for pool in pools:
                        assert pool.dirty_batch == (0 if clear else B)
        assert opt.calls["dense"] == 0 and opt.calls.get("union", 0) == 0 and opt.calls["rows"] == calls, opt.calls
        for n, p in tables.items():
            assert torch.equal(p.detach()[~ever[n]], init[n][~ever[n]]), n
            st = opt.state[id(p)]
            if rule == "adagrad":
                _close("%s sum %s" % (rule, n), st["s"][0], state[n]["sum"], STATE_ATOL)
            if rule == "adam":
                _close("%s m %s" % (rule, n), st["s"][0], state[n]["m"], STATE_ATOL)
                _close("%s v %s" % (rule, n), st["s"][1], state[n]["v"], STATE_ATOL)
    finally:
        ops.config.reuse_grad_buffers = old
        ops.config.track_touched_rows = False


def test_table_shared_by_a_bag_feature_and_a_padded_feature_steps_over_the_union():
    from recbox_amd import ops
    layer, feats = _layer(shared=True)
    table = layer.embed_dict["b"].weight
    opt, hp = _make("adagrad", [table])
    ref = table.detach().clone()
    state = {"step": 0, "sum": torch.zeros_like(table)}
    try:
        for k in range(3):
            gen = torch.Generator().manual_seed(90 + k)
            ids, offsets = _ragged(150, 64, gen, lo=0)                     # the bags name rows below 150 ...
            x = {"b": torch.randint(150, 300, (64,), generator=gen).cuda(),  # ... the padded feature rows above
                 "hist_b": ops.Bags(ids.cuda(), offsets.cuda())}
            opt.zero_grad()
            out = layer(x, feats, squeeze_dim=True)
            (out * out).sum().backward()
            g = table.grad.detach().clone()
            rows = (g != 0).any(dim=1).nonzero().reshape(-1)
            assert int((rows < 150).sum()) > 0 and int((rows >= 150).sum()) > 0
            opt.step()
            _reference_step("adagrad", ref, g, rows, state, hp)
            _close("shared table step %d" % k, table.detach(), ref, TABLE_ATOL)
        assert opt.calls.get("union", 0) > 0 and opt.calls["rows"] == 0, opt.calls
    finally:
        ops.config.track_touched_rows = False


# ---- one captured step --------------------------------------------------------------------------------------------------------
def test_captured_step_with_capturable_adam_and_clear_grads_replays_like_eager_steps():
    """forward, loss, backward and SparseAdam(capturable=True, clear_grads=True).step() in ONE graph over a bag-fed layer:
    three warm-up steps and three replays on one resident batch equal six eager steps of the by-value optimiser."""
    from recbox_amd import ops, optim
    from recbox_amd.graph import GraphedStep
    x, _, dY = _layer_batch(400, 77)
    old_check = ops.config.check_ids
    ops.config.check_ids = False

    def step_of(layer, feats, opt):
        def fn():
            opt.zero_grad()
            out = layer(x, feats, squeeze_dim=True)
            loss = (out * dY).sum()
            loss.backward()
            opt.step()
            return loss
        return fn

    try:
        n_warm, n_replay = 3, 3
        eager, feats_e = _layer()
        tables_e = [eager.embed_dict[f.name].weight for f in feats_e]
        opt_e = optim.SparseAdam(tables_e, lr=0.01)
        fn_e = step_of(eager, feats_e, opt_e)
        for _ in range(n_warm + n_replay):
            fn_e()
        assert opt_e.calls["dense"] == 0
        graphed, feats_g = _layer()
        tables_g = [graphed.embed_dict[f.name].weight for f in feats_g]
        opt_g = optim.SparseAdam(tables_g, lr=0.01, capturable=True, clear_grads=True)
        step = GraphedStep(step_of(graphed, feats_g, opt_g), warmup=n_warm, reuse_grads="all")
        for _ in range(n_replay):            # (the capture pass itself does not execute: the device counter stands at n_warm)
            step()
        torch.cuda.synchronize()
        ops.check_deferred_ids()
        assert float(opt_g._dev["t"]) == n_warm + n_replay
        assert opt_g.calls["dense"] == 0 and all(pool.dirty_batch == 0 for pool in _pools_of(graphed))
        for pe, pg in zip(tables_e, tables_g):
            _close("captured table %d rows" % pe.shape[0], pg.detach(), pe.detach(), TABLE_ATOL)
            for k in range(2):
                _close("captured state%d %d rows" % (k + 1, pe.shape[0]), opt_g.state[id(pg)]["s"][k], opt_e.state[id(pe)]["s"][k],
                       STATE_ATOL)
            assert int(torch.count_nonzero(pg.grad)) == 0
    finally:
        ops.config.check_ids = old_check
        ops.config.track_touched_rows = False
