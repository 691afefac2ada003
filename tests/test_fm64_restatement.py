"""CPU checks of the float64 FM restatement (oracle/fm64.py) that the GPU tests of tests/test_gpu_fm_dims.py compare the
fused FM kernels with: it equals torch autograd on the oracle model in float64, and its per-element bound is tight enough
to catch one lost lookup -- in a row looked up once and in the hottest row of a 65 536-sample batch -- and one lost
512-chunk window of the long fix-up in a row that 80 % of a field's 65 536 lookups hit."""
from collections import OrderedDict

import pytest
import torch

from oracle.fm64 import Table, bound_ratio, fm_body64
from test_oracle_golden import _FM


def _schema(vocabs, n_num, shared=None):
    feats = OrderedDict()
    for i in range(n_num):
        feats["I%d" % i] = {"source": "", "type": "numeric"}
    for i, v in enumerate(vocabs):
        feats["C%d" % i] = {"source": "", "type": "categorical", "vocab_size": v, "padding_idx": 0}
    if shared is not None:
        feats["S"] = {"source": "", "type": "categorical", "vocab_size": vocabs[shared], "padding_idx": 0,
                      "share_embedding": "C%d" % shared}
    return _FM(feats)


def _batch(fm, B, gen, pad_frac=0.05):
    X = OrderedDict()
    for name, spec in fm.features.items():
        if spec["type"] == "numeric":
            X[name] = torch.rand(B, generator=gen, dtype=torch.float64) * 2 - 0.5
        else:
            v = spec["vocab_size"]
            ids = torch.randint(1, v, (B,), generator=gen)
            ids[torch.rand(B, generator=gen) < pad_frac] = 0
            X[name] = ids.double()
    return X


def _fields_of(model, fm, X):
    """fields of fm_body64 from a model that holds the reference's parameter layout (embedding_layer / fm.lr_layer)."""
    emb = model.embedding_layer.embedding_layer.embedding_layers
    lr = model.fm.lr_layer.embedding_layer.embedding_layer.embedding_layers
    tables = {}

    def table(module, is_lr):
        if id(module) not in tables:
            w = module.weight.detach().cpu()
            if isinstance(module, torch.nn.Embedding):
                tables[id(module)] = Table(w, module.padding_idx)
            else:                                       # numeric: [D] embedding weight, scalar LR weight
                tables[id(module)] = Table(w.view(()) if is_lr else w.view(-1))
        return tables[id(module)]

    fields = []
    for name, spec in fm.features.items():
        fields.append((spec["type"], X[name], table(emb[name], False), table(lr[name], True)))
    return fields, tables


def _ref_model(fm, D, seed):
    from oracle import torch_ref as R
    ref = R.RefFMModel(fm, D).double()
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in ref.parameters():
            p.copy_(torch.randn(p.shape, generator=gen, dtype=torch.float64) * 0.3)
        for m in ref.modules():
            if isinstance(m, torch.nn.Embedding) and m.padding_idx is not None:
                m.weight[m.padding_idx].zero_()
            if isinstance(m, torch.nn.Linear):          # the oracle casts x to float32; keep the float64 model in float64
                m.register_forward_pre_hook(lambda mod, args: (args[0].double(),))
    return ref


@pytest.mark.parametrize("D,B,n_num,shared", [(1, 5, 2, None), (7, 33, 3, 1), (10, 64, 13, 0), (16, 9, 0, None)])
def test_restatement_equals_autograd_on_the_oracle_model_in_float64(D, B, n_num, shared):
    fm = _schema([2, 3, 11, 40], n_num, shared)
    ref = _ref_model(fm, D, seed=D)
    gen = torch.Generator().manual_seed(100 + D)
    X = _batch(fm, B, gen, pad_frac=0.2)
    g = torch.randn(B, generator=gen, dtype=torch.float64)
    logit = ref(X).view(-1)
    logit.backward(g)
    fields, tables = _fields_of(ref, fm, X)
    want, a_logit, grads, (dbias, a_bias) = fm_body64(fields, ref.fm.lr_layer.bias.detach(), g)
    assert torch.allclose(want, logit.detach(), rtol=1e-12, atol=1e-12)
    assert bool((a_logit >= want.abs() - 1e-12).all())
    assert torch.allclose(dbias, ref.fm.lr_layer.bias.grad.view(()), rtol=1e-12, atol=1e-12)
    seen = set()
    for m in ref.modules():
        if not isinstance(m, (torch.nn.Embedding, torch.nn.Linear)) or id(m) in seen:
            continue
        seen.add(id(m))
        _, w, A = grads[id(tables[id(m)])]
        got = m.weight.grad.view(w.shape)
        assert torch.allclose(w, got, rtol=1e-12, atol=1e-12), m
        assert bool((A >= w.abs() - 1e-12).all())
        assert bound_ratio(got.float(), w, A) <= 1.0          # float32 rounding of the exact value is inside the bar


def _one_lookup_contribution(fields, g, f, b):
    """dV[id_fb] of lookup (f, b) alone: g_b (S_b - e_f[b])."""
    _, _, grads, _ = fm_body64(fields, None, g * (torch.arange(g.numel()) == b).double())
    table = fields[f][2]
    return grads[id(table)][1][fields[f][1][b].long()]


def test_bound_rejects_a_lost_lookup_in_a_row_looked_up_once():
    fm = _schema([2, 3, 5000], 13)
    ref = _ref_model(fm, 10, seed=1)
    gen = torch.Generator().manual_seed(2)
    B = 257
    X = _batch(fm, B, gen)
    g = torch.randn(B, generator=gen, dtype=torch.float64)
    fields, _ = _fields_of(ref, fm, X)
    f = len(fields) - 1                                  # the 5000-row table
    ids = X["C2"].long()
    counts = torch.bincount(ids, minlength=5000)
    b = int(((counts[ids] == 1) & (ids != 0)).nonzero()[0])
    _, _, grads, _ = fm_body64(fields, None, g)
    table, want, A = grads[id(fields[f][2])]
    r = int(ids[b])
    assert bound_ratio(want[r].float(), want[r], A[r]) <= 1.0
    lost = want[r] - _one_lookup_contribution(fields, g, f, b)
    assert bound_ratio(lost, want[r], A[r]) > 1.0


def test_bound_rejects_a_lost_lookup_in_the_hottest_row_at_full_batch():
    """Rows of a 3-row table at B = 65 536 sum ~31 000 lookups each (the bench schema's smallest Criteo table)."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    fm = _schema([3, 4, 1460, 5683], 13)
    ref = _ref_model(fm, 16, seed=3)
    gen = torch.Generator().manual_seed(4)
    B = 65536
    X = _batch(fm, B, gen)
    g = torch.randn(B, generator=gen, dtype=torch.float64)
    fields, _ = _fields_of(ref, fm, X)
    f = 13                                               # the 3-row table
    _, _, grads, _ = fm_body64(fields, None, g)
    _, want, A = grads[id(fields[f][2])]
    ids = X["C0"].long()
    r = int(torch.bincount(ids[ids != 0]).argmax())
    assert int((ids == r).sum()) > 30000
    b = int((ids == r).nonzero()[0])
    lost = want[r] - _one_lookup_contribution(fields, g, f, b)
    assert bound_ratio(lost, want[r], A[r]) > 1.0


def hot_id_batch(B, seed, hot_frac=0.8, vocab=10000, n_fields=4):
    """ids of the hot-id case: ``n_fields`` columns of ids in ``vocab`` rows, ``hot_frac`` of every column's lookups on
    id 7, the rest uniform over the other rows (5 % of those the padding id 0)."""
    gen = torch.Generator().manual_seed(seed)
    cols = []
    for _ in range(n_fields):
        ids = torch.randint(1, vocab, (B,), generator=gen)
        ids[torch.rand(B, generator=gen) < 0.05] = 0
        ids[torch.rand(B, generator=gen) < hot_frac] = 7
        cols.append(ids)
    return cols


def test_bound_rejects_a_lost_window_of_the_long_fixup_in_a_hot_row():
    """The GPU hot-id case: four fields, each over its own 10 000-row table, 80 % of every field's lookups on one row
    (~52 000 lookups: a chain of ~3 300 chunks of 16 sorted pairs).  Losing one window of the long fix-up (512 chunks:
    8 192 lookups) of that chain must break the bound."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    D, B = 16, 65536
    gen = torch.Generator().manual_seed(5)
    fields = [("numeric", torch.rand(B, generator=gen, dtype=torch.float64),
               Table(torch.randn(D, generator=gen, dtype=torch.float64) * 0.3), Table(torch.randn((), generator=gen)))]
    cols = hot_id_batch(B, 6)
    tables = []
    for c in cols:
        hot = Table(torch.randn(10000, D, generator=gen, dtype=torch.float64) * 0.3, pad=0)
        hot.weight[0] = 0
        hot_lr = Table(torch.randn(10000, 1, generator=gen, dtype=torch.float64) * 0.3, pad=0)
        tables.append(hot)
        fields.append(("categorical", c, hot, hot_lr))
    g = torch.randn(B, generator=gen, dtype=torch.float64)
    _, _, grads, _ = fm_body64(fields, None, g)
    hot = tables[0]
    _, want, A = grads[id(hot)]
    assert int((cols[0] == 7).sum()) > 3200 * 16
    # the first 8 192 lookups of the hot row: their contribution g_b (S_b - v_7) to row 7
    window = (cols[0] == 7).nonzero().view(-1)[:8192]
    S = torch.zeros(B, D, dtype=torch.float64)
    for kind, col, emb, _ in fields:
        S += emb.weight[col.long()] if kind == "categorical" else col.float().double()[:, None] * emb.weight.view(1, -1)
    contrib = (g[window][:, None] * (S[window] - hot.weight[7])).sum(0)
    assert bound_ratio(want[7].float(), want[7], A[7]) <= 1.0
    assert bound_ratio(want[7] - contrib, want[7], A[7]) > 1.0
