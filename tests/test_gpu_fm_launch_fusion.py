"""The fused FM step's merged head launch (ops.config.fm_fuse_launches, on by default) against the float64 restatement of
oracle/fm64.py and, bit for bit, against the same step through the separate entry points:

  head    rbx_fm_head: one launch whose workgroups are id-compaction tiles (compact_ids_tile) or re-zero blocks
          (rezero_rows_block), instead of rbx_fm_rezero followed by rbx_fm_sort_phases(FM_SORT_IDS).  Taken by a step with
          persistent gradients (config.reuse_grad_buffers) whose previous step had the same batch size.

(The numeric features' final sums stay fm_numeric_final_kernel, a launch of their own, in both arms.)

The model is the smallest that has every part: tier-A tables of 7 and 300 rows, a tier-B table of 5000 rows, one numeric
feature; D = 16 and D = 8 (the forward's non-quad form).  Batches: 1; 2047 and 2049 (a short last tier-A block of 2048
samples, a last compaction tile shorter than cid_ts); 4096 with every id of the 5000-row table equal (one run of the sorted
reduce over all its chunks: the long fix-up); 4096 with all of them distinct (both fix-ups empty).  Id columns are separate
contiguous tensors ("cols": the compaction walks samples fastest) or the columns of one [B, 4] tensor ("rows": FIELD_FAST).
Tolerances: those of tests/test_gpu_fm_dims.py (check_against_restatement, C = oracle.fm64.C_BOUND)."""
from collections import OrderedDict

import pytest
import torch

from test_gpu_fm_dims import _features, _holders, _model, check_against_restatement

pytestmark = pytest.mark.gpu

VOCABS = [7, 300, 5000]
CASES = [(1, "random", "cols"), (2047, "random", "rows"), (2049, "random", "cols"), (2049, "random", "rows"),
         (4096, "equal", "rows"), (4096, "distinct", "cols")]


@pytest.fixture(autouse=True)
def _persistent_grads(monkeypatch):
    from recbox_amd import ops
    monkeypatch.setattr(ops.config, "reuse_grad_buffers", True)
    monkeypatch.setattr(ops.config, "fm_fuse_launches", True)


def _batch(B, kind, layout, seed):
    """CPU inputs of one step, float64 as the ranking loader hands them over: I0, C0 (7 rows), C1 (300), C2 (5000)."""
    gen = torch.Generator().manual_seed(seed)
    cols = [torch.rand(B, generator=gen, dtype=torch.float64) * 2 - 0.5]
    for v in VOCABS:
        ids = torch.randint(1, v, (B,), generator=gen)
        ids[torch.rand(B, generator=gen) < 0.05] = 0
        cols.append(ids)
    if kind == "equal":
        cols[3] = torch.full((B,), 17 + seed % 5, dtype=torch.int64)
    elif kind == "distinct":
        cols[3] = torch.randperm(4999, generator=gen)[:B] + 1
    names = ["I0", "C0", "C1", "C2"]
    if layout == "rows":
        block = torch.stack([c.double() for c in cols], dim=1)
        return OrderedDict((n, block[:, i]) for i, n in enumerate(names))
    return OrderedDict((n, c.double().contiguous()) for n, c in zip(names, cols))


def _on_gpu(X):
    if not X["I0"].is_contiguous():                     # the columns of one batch tensor stay that on the device
        block = torch.stack(list(X.values()), dim=1).cuda()
        return OrderedDict((n, block[:, i]) for i, n in enumerate(X))
    return OrderedDict((n, c.cuda()) for n, c in X.items())


def _step(model, X, g, presorted=None):
    for p in model.parameters():
        p.grad = None
    logit = model.logits(_on_gpu(X), presorted=presorted)
    logit.backward(g.cuda().view(-1, 1))
    torch.cuda.synchronize()
    return logit.detach()


def _grads(model):
    return OrderedDict((n, p.grad.detach().clone()) for n, p in model.named_parameters())


def _count_head_calls(monkeypatch):
    """Every rbx_fm_head call as (re-zero workspace, sort workspace) addresses."""
    from recbox_amd import ops
    calls = []
    real = ops.lib.rbx_fm_head

    def spy(*a):
        calls.append((getattr(a[4], "value", a[4]), getattr(a[6], "value", a[6])))
        return real(*a)

    monkeypatch.setattr(ops.lib, "rbx_fm_head", spy, raising=False)
    return calls


def _rows_only_in(X_then, X_now, name="C2"):
    then, now = set(X_then[name].long().tolist()), set(X_now[name].long().tolist())
    return torch.tensor(sorted(then - now), dtype=torch.int64)


def _assert_rows_zero(model, rows, tag):
    emb, lr = _holders(model)
    for what, holder in (("emb", emb), ("lr", lr)):
        got = holder["C2"].weight.grad[rows.cuda()]
        assert int(torch.count_nonzero(got)) == 0, "%s: %s C2: rows of the earlier step were not cleared" % (tag, what)


@pytest.mark.parametrize("D", [16, 8])
@pytest.mark.parametrize("B,kind,layout", CASES)
def test_two_steps_against_float64_and_the_separate_launches(monkeypatch, D, B, kind, layout):
    """Two consecutive steps with different ids on persistent gradients.  After the second: every gradient within the bound
    of the float64 restatement (rows no lookup of THIS step reached exactly zero -- the head launch cleared the first
    step's), and bit-equal to the same two steps through rbx_fm_rezero + rbx_fm_sort_phases."""
    from recbox_amd import ops
    fm = _features(VOCABS, 1)
    X1, X2 = _batch(B, kind, layout, seed=11 + B), _batch(B, kind, layout, seed=12 + B)
    g1 = torch.randn(B, generator=torch.Generator().manual_seed(B))
    g2 = torch.randn(B, generator=torch.Generator().manual_seed(B + 1))
    tag = "D%d B%d %s %s" % (D, B, kind, layout)

    calls = _count_head_calls(monkeypatch)
    fused = _model(fm, D, True, seed=D)
    _step(fused, X1, g1)
    first_fused = _grads(fused)
    assert calls == [], "the first step has nothing to clear: id compaction alone"
    logit = _step(fused, X2, g2)
    assert len(calls) == 1, "the second step's head is one rbx_fm_head call"
    check_against_restatement(fused, fm, X2, g2, logit, tag + " fused")
    gone = _rows_only_in(X1, X2)
    if gone.numel():
        _assert_rows_zero(fused, gone, tag)
    second_fused = _grads(fused)

    monkeypatch.setattr(ops.config, "fm_fuse_launches", False)
    plain = _model(fm, D, True, seed=D)
    _step(plain, X1, g1)
    first_plain = _grads(plain)
    logit = _step(plain, X2, g2)
    assert len(calls) == 1, "fm_fuse_launches = False must not call rbx_fm_head"
    check_against_restatement(plain, fm, X2, g2, logit, tag + " separate")
    second_plain = _grads(plain)
    for name in second_fused:
        assert torch.equal(first_fused[name], first_plain[name]), "%s: step 1: %s differs bit for bit" % (tag, name)
        assert torch.equal(second_fused[name], second_plain[name]), "%s: step 2: %s differs bit for bit" % (tag, name)


@pytest.mark.parametrize("D", [16, 8])
@pytest.mark.parametrize("B,kind,layout", [(2049, "random", "rows"), (4096, "equal", "cols")])
def test_step_after_a_presorted_step_clears_the_other_workspace(monkeypatch, D, B, kind, layout):
    """own sort, presorted (FM.presort: the sorted ids live in the caller's workspace), own sort: the third step's head
    clears the rows named by the PRESORTED workspace while it compacts ids into the pool's -- two different buffers."""
    from recbox_amd import ops
    fm = _features(VOCABS, 1)
    Xs = [_batch(B, kind, layout, seed=21 + B + k) for k in range(3)]
    gs = [torch.randn(B, generator=torch.Generator().manual_seed(3 * B + k)) for k in range(3)]
    tag = "presorted D%d B%d %s" % (D, B, kind)

    def three_steps(model):
        _step(model, Xs[0], gs[0])
        pre = model.presort(_on_gpu(Xs[1]))
        torch.cuda.synchronize()
        _step(model, Xs[1], gs[1], presorted=pre)
        logit = _step(model, Xs[2], gs[2])
        check_against_restatement(model, fm, Xs[2], gs[2], logit, tag)
        gone = _rows_only_in(Xs[1], Xs[2])
        if gone.numel():
            _assert_rows_zero(model, gone, tag)
        return pre, _grads(model)

    calls = _count_head_calls(monkeypatch)
    pre, fused = three_steps(_model(fm, D, True, seed=D))
    assert len(calls) == 1 and calls[0][0] == pre.ws.data_ptr() and calls[0][1] != calls[0][0], \
        "the third step's head reads the presorted workspace and writes the pool's"
    monkeypatch.setattr(ops.config, "fm_fuse_launches", False)
    _, plain = three_steps(_model(fm, D, True, seed=D))
    assert len(calls) == 1
    for name in fused:
        assert torch.equal(fused[name], plain[name]), "%s: %s differs bit for bit" % (tag, name)


def test_more_descriptors_than_one_head_launch_carries_keeps_the_two_launches(monkeypatch):
    """56 sorted tables: 56 re-zero descriptors (48 B) + 56 compaction descriptors (24 B) = 4032 B, more than the 3840 B the
    merged head launch carries in its arguments, so rbx_fm_head issues the re-zero and the compaction as two launches.  Same
    checks as above: float64 bound, cleared rows, bit-equal to the separate entry points."""
    from recbox_amd import ops
    vocabs = [4200 + i for i in range(56)]
    B, D = 300, 16
    fm = _features(vocabs, 1)

    def batch(seed):
        gen = torch.Generator().manual_seed(seed)
        X = OrderedDict([("I0", torch.rand(B, generator=gen, dtype=torch.float64) * 2 - 0.5)])
        for i, v in enumerate(vocabs):
            X["C%d" % i] = torch.randint(1, v, (B,), generator=gen).double()
        return X

    X1, X2 = batch(51), batch(52)
    g1 = torch.randn(B, generator=torch.Generator().manual_seed(53))
    g2 = torch.randn(B, generator=torch.Generator().manual_seed(54))
    calls = _count_head_calls(monkeypatch)
    fused = _model(fm, D, True, seed=7)
    _step(fused, X1, g1)
    logit = _step(fused, X2, g2)
    assert len(calls) == 1
    check_against_restatement(fused, fm, X2, g2, logit, "56 tables fused")
    _assert_rows_zero(fused, _rows_only_in(X1, X2), "56 tables")
    monkeypatch.setattr(ops.config, "fm_fuse_launches", False)
    plain = _model(fm, D, True, seed=7)
    _step(plain, X1, g1)
    _step(plain, X2, g2)
    assert len(calls) == 1
    for (name, a), (_, b) in zip(_grads(fused).items(), _grads(plain).items()):
        assert torch.equal(a, b), "56 tables: %s differs bit for bit" % name


def _bound_tables(model, X):
    """The model's fused-call descriptors (ops._FmTables) pointed at batch X, with gradient buffers of their own."""
    from recbox_amd import ops
    emb = model.embedding_layer.embedding_layer
    lr = model.fm.lr_layer.embedding_layer.embedding_layer
    _, values, plan, _ = emb.plan_for(X)
    _, _, lplan, _ = lr.plan_for(X)
    tb = ops._FmTables(plan.plan, lplan.plan, [m.weight for m in plan.modules], [m.weight for m in lplan.modules])
    B, keep = tb.bind_inputs(values)
    return tb, B, keep


@pytest.mark.parametrize("layout", ["cols", "rows"])
def test_head_entry_point_status_word_and_stores(layout):
    """rbx_fm_head through the C ABI: it clears exactly the rows the previous sort names and leaves the compact id matrix
    rbx_fm_sort_phases leaves; an id outside its table raises the status word, valid ids leave it alone."""
    from recbox_amd import ops
    lib, ptr, stream = ops.lib, ops._ptr, ops._stream
    B = 2049
    fm = _features(VOCABS, 1)
    model = _model(fm, 16, True, seed=5)
    X1, X2 = _on_gpu(_batch(B, "random", layout, seed=31)), _on_gpu(_batch(B, "random", layout, seed=32))
    tb, _, keep1 = _bound_tables(model, X1)
    grads = [torch.ones_like(p) for p in tb.params]
    tb.bind(grads)
    nbytes = lib.rbx_fm_bwd_workspace_size(tb.ea, tb.la, tb.n, B)
    assert nbytes > 0
    prev = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    ops.check(lib.rbx_fm_sort(tb.ea, tb.la, tb.n, B, ptr(prev), nbytes, None, stream()))     # the "previous step's" pairs
    torch.cuda.synchronize()

    def head(X, fused):
        for gr in grads:
            gr.fill_(1.0)
        tb2, _, keep = _bound_tables(model, X)
        tb2.bind(grads)
        ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        if fused:
            ops.check(lib.rbx_fm_head(tb2.ea, tb2.la, tb2.n, B, ptr(prev), nbytes, ptr(ws), nbytes, ptr(status), stream()))
        else:
            ops.check(lib.rbx_fm_rezero(tb2.ea, tb2.la, tb2.n, B, ptr(prev), nbytes, stream()))
            ops.check(lib.rbx_fm_sort_phases(tb2.ea, tb2.la, tb2.n, B, ptr(ws), nbytes, ptr(status), 1, stream()))
        torch.cuda.synchronize()
        del keep
        return ws, int(status.item()), [gr.clone() for gr in grads]

    ws_f, st_f, g_f = head(X2, True)
    ws_s, st_s, g_s = head(X2, False)
    assert st_f == 0 and st_s == 0
    assert torch.equal(ws_f, ws_s), "the compact id matrix differs from rbx_fm_sort_phases'"
    for a, b in zip(g_f, g_s):
        assert torch.equal(a, b)
    # the 5000-row table (tier B): exactly the rows X1 looked up are cleared; tier-A tables are not the re-zero's business
    emb, lr = _holders(model)
    looked = torch.unique(X1["C2"].long())
    for holder in (emb, lr):
        k = [i for i, p in enumerate(tb.params) if p is holder["C2"].weight][0]
        want = torch.ones_like(g_f[k])
        want[looked] = 0
        assert torch.equal(g_f[k][1:], want[1:])       # (row 0 is the padding id: no sorted pair names it)
    bad = OrderedDict((n, c.clone()) for n, c in _on_gpu(_batch(B, "random", "cols", seed=33)).items())
    bad["C2"][B - 1] = 5000.0                        # one past the last row, in the last (short) compaction tile
    _, st_bad, _ = head(bad, True)
    assert st_bad != 0, "an id outside its table must raise the status word through rbx_fm_head"
    del keep1


def test_head_entry_point_with_an_empty_batch():
    """batch == 0: RBX_OK, and nothing is read or written (no workspace, no status word given)."""
    from recbox_amd import ops
    fm = _features(VOCABS, 1)
    model = _model(fm, 16, True, seed=6)
    tb, _, keep = _bound_tables(model, _on_gpu(_batch(4, "random", "cols", seed=41)))
    grads = [torch.ones_like(p) for p in tb.params]
    tb.bind(grads)
    assert ops.lib.rbx_fm_head(tb.ea, tb.la, tb.n, 0, None, 0, None, 0, None, ops._stream()) == 0
    torch.cuda.synchronize()
    for gr in grads:
        assert bool((gr == 1).all())
    del keep
