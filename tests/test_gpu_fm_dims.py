"""The FM model body -- fused (rbx_fm_fwd / rbx_fm_bwd) and layer-composed -- against the float64 restatement of
oracle/fm64.py at every embedding dim the fused kernels dispatch, with the per-element bound
|got - want| <= C eps32 A + tiny (A: the same sums over absolute values, C = oracle.fm64.C_BOUND for the whole file).
The kernels are driven by ``logit.backward(g)`` with a random g (exact in float64), the bench's sigmoid + BCE chain once.
Rows that no lookup reached and padding rows have A = 0: their gradient must be exactly zero.

Which instantiation each dim selects (units = D / 4 when D % 4 == 0, else D; G = the next power of two >= units):
  forward      dispatch_fm_fwd: fm_fused_fwd_kernel<G, 1, D % 4 == 0, DT>, DT = the ids' dtype when every column shares it
               (float64 / int64), -1 (generic decode) otherwise; refused when G > 64 (non-vector D > 64, vector D > 256)
  tier A       tables of <= 4096 rows while their gradients fit 1 M floats, D <= 64 only (kTaMaxDim), ta_dispatch_bwd:
               vector G <= 4 (D = 4, 8, 12, 16): ta_reduce_lds_kernel<G>, otherwise ta_reduce_kernel<G, VEC>; then
               ta_final_kernel<G, VEC> (vector G at most 16)
  tier B       dispatch_reduce: segment_reduce_kernel / segment_fixup_short_kernel / segment_fixup_long_kernel
               <FmPolicy, G, 1, VEC> (G <= 64; NV > 1 only for dims the forward refuses)
  numeric      num_blocks_form (D % 4 == 0, <= kTaNumMax = 32 numeric features, 512 samples' LDS <= 96 KB): their partials
               ride in ta_reduce_lds_kernel's launch when that runs, else fm_numeric_blocks_kernel; otherwise
               fm_numeric_partial_kernel; then fm_numeric_final_kernel
  D      fwd <G,VEC>   tier A                          tier B           numeric (13 features)
  1      <1,false>     reduce<1,false>  final<1,false>   <1,1,false>      partial
  2      <2,false>     reduce<2,false>  final<2,false>   <2,1,false>      partial
  3      <4,false>     reduce<4,false>  final<4,false>   <4,1,false>      partial
  4      <1,true>      lds<1>           final<1,true>    <1,1,true>       in the lds launch
  7      <8,false>     reduce<8,false>  final<8,false>   <8,1,false>      partial
  8      <2,true>      lds<2>           final<2,true>    <2,1,true>       in the lds launch
  10     <16,false>    reduce<16,false> final<16,false>  <16,1,false>     partial
  12     <4,true>      lds<4>           final<4,true>    <4,1,true>       in the lds launch
  17     <32,false>    reduce<32,false> final<32,false>  <32,1,false>     partial
  20, 24 <8,true>      reduce<8,true>   final<8,true>    <8,1,true>       blocks
  33     <64,false>    reduce<64,false> final<64,false>  <64,1,false>     partial
  36..64 <16,true>     reduce<16,true>  final<16,true>   <16,1,true>      partial (1 numeric feature at 40, 44: blocks)
  68     <32,true>     -- (D > 64)                       <32,1,true>      partial
  65, 132, 256, 260: the fused body refuses them (RBX_ERR_UNSUPPORTED from rbx_fm_fwd / rbx_fm_bwd: D > kFmMaxDim = 128,
  or no forward instantiation) and fm_fused_takes_dim() lets the model compose the layers, as with fused=False.  At
  132 .. 256 (vector G = 64) the sorted tier left rows of a few thousand lookups up to 2 % off: kept as the strict
  expected failure test_fused_body_at_dim_132_with_hot_rows.  The three kernels of rbx_segreduce.h are NOT the cause:
  test_gpu_embed_dims.py holds their <64, 1, true> form to the same bound with GenericPolicy and DotPolicy, hot rows
  split over workgroups included (3 % of the bound).  With the refusal lifted on a scratch build, the xfail case fails on
  ONE gradient: the 3-row table's embedding gradient (3 700 x the bound); that table's LR gradient -- the count column of
  the same summaries --, the 2-row and 5000-row tables' gradients and the logit meet it (under 3 % of the bound).  So the
  forward, the count column and the sums of g S are cleared too; what remains is FmPolicy::flush's - cnt * w_r term (the
  prefetched row) where two hot rows of one table are adjacent chains.  100 (25 float4s, G = 32) stays fused.
Fields that share an embedding table but not their LR tables (share_embedding; the LR layer never shares) compose the
layers too (ops.fm_fused refuses them): the fused backward summed their LR gradients into one of the tables."""
from collections import OrderedDict

import pytest
import torch

from conftest import _note
from oracle.fm64 import Table, bound_ratio, fm_body64
from test_fm64_restatement import hot_id_batch
from test_oracle_golden import _FM

pytestmark = pytest.mark.gpu

DIMS = [1, 2, 3, 4, 7, 8, 10, 12, 17, 20, 24, 33, 36, 40, 48, 64, 68, 132, 256]
GRID_VOCABS = [2, 3, 300, 4000, 5000, 70000, 1000000]   # tier A: 2 .. 4000 rows (as the budget allows), tier B: 5000 ..
NO_PAD = {70000}                                        # one table without a padding row


def _features(vocabs, n_num, shared=None, no_pad=()):
    feats = OrderedDict()
    for i in range(n_num):
        feats["I%d" % i] = {"source": "", "type": "numeric"}
    for i, v in enumerate(vocabs):
        spec = {"source": "", "type": "categorical", "vocab_size": v}
        if v not in no_pad:
            spec["padding_idx"] = 0
        feats["C%d" % i] = spec
    for k, target in enumerate(shared or ()):
        feats["S%d" % k] = dict(feats["C%d" % target], share_embedding="C%d" % target)
    return _FM(feats)


def _batch(fm, B, seed, id_dtype, pad_frac=0.05):
    gen = torch.Generator().manual_seed(seed)
    X = OrderedDict()
    for name, spec in fm.features.items():
        if spec["type"] == "numeric":
            X[name] = torch.rand(B, generator=gen, dtype=torch.float64) * 2 - 0.5
        else:
            v = spec["vocab_size"]
            ids = torch.randint(0 if v == 2 else 1, v, (B,), generator=gen)
            if "padding_idx" in spec:
                ids[torch.rand(B, generator=gen) < pad_frac] = 0
            X[name] = ids.to(id_dtype)
    return X


def _model(fm, D, fused, seed):
    from recbox_amd.ranking.pytorch.models import FM
    model = FM(fm, D, fused=fused).cuda()
    gen = torch.Generator(device="cuda").manual_seed(seed)
    with torch.no_grad():
        for _, p in model.named_parameters():
            p.copy_(torch.randn(p.shape, generator=gen, device="cuda") * 0.1)
        for m in model.modules():
            if isinstance(m, torch.nn.Embedding) and m.padding_idx is not None:
                m.weight[m.padding_idx].zero_()
    return model


def _holders(model):
    return (model.embedding_layer.embedding_layer.embedding_layers,
            model.fm.lr_layer.embedding_layer.embedding_layer.embedding_layers)


def check_against_restatement(model, fm, X, g, logit, tag):
    """Logit, bias gradient and every table / weight gradient of ``model`` after ``logit.backward(g)`` against fm_body64,
    on the rows the batch looked up (compact copies of those rows only); every other row's gradient must be zero."""
    emb, lr = _holders(model)
    # a field's LR table is compacted to the rows of its embedding table (every field that shares it): one id column
    # serves both, and rows only the other field looked up must keep a zero LR gradient
    uses = {}
    for name, spec in fm.features.items():
        if spec["type"] != "numeric":
            uses.setdefault(id(emb[name]), []).append(X[name].long().cpu())
    for name, spec in fm.features.items():
        if spec["type"] != "numeric":
            uses[id(lr[name])] = uses[id(emb[name])]
    tables = {}

    def table(module, is_lr):
        t = tables.get(id(module))
        if t is None:
            if isinstance(module, torch.nn.Embedding):
                rows = torch.unique(torch.cat(uses[id(module)]))
                t = Table(module.weight.detach()[rows.cuda()].cpu(), None)
                if module.padding_idx is not None and bool((rows == module.padding_idx).any()):
                    t.pad = int((rows == module.padding_idx).nonzero())
                t.rows = rows
            else:
                w = module.weight.detach().cpu()
                t = Table(w.view(()) if is_lr else w.view(-1))
                t.rows = None
            t.module = module
            tables[id(module)] = t
        return t

    fields = []
    for name, spec in fm.features.items():
        te, tl = table(emb[name], False), table(lr[name], True)
        col = X[name].cpu()
        if spec["type"] != "numeric":
            col = torch.searchsorted(te.rows, col.long())
        fields.append((spec["type"], col, te, tl))
    bias = model.fm.lr_layer.bias
    want, a_logit, grads, (dbias, a_bias) = fm_body64(fields, bias.detach().cpu(), g.double().cpu())
    ratios = {"logit": bound_ratio(logit.view(-1), want, a_logit)}
    ratios["bias"] = bound_ratio(bias.grad.view(()), dbias, a_bias)
    names = {}
    for holder, kind in ((emb, "emb"), (lr, "lr")):
        for name, module in holder.items():
            names.setdefault(id(module), "%s %s" % (kind, name))
    for t, w, A in grads.values():
        p = t.module.weight
        got = p.grad if p.grad is not None else torch.zeros_like(p)
        what = names[id(t.module)]
        if t.rows is None:
            ratios[what] = bound_ratio(got, w, A)
            continue
        rows = t.rows.cuda()
        ratios[what] = bound_ratio(got[rows], w, A)
        rest = got.detach().clone()
        rest[rows] = 0
        n_bad = int(torch.count_nonzero(rest))
        assert n_bad == 0, "%s: %s: %d gradient entries outside the looked-up rows" % (tag, what, n_bad)
    for what, r in ratios.items():
        _note("%s %s (err / bound)" % (tag, what), r, 1.0)
    worst = max(ratios.items(), key=lambda kv: kv[1])
    assert worst[1] <= 1.0, "%s: %s error is %.3g x the bound (all: %s)" % (
        tag, worst[0], worst[1], ", ".join("%s %.2g" % kv for kv in sorted(ratios.items(), key=lambda kv: -kv[1])[:6]))
    return ratios


def _step(model, X, g):
    for p in model.parameters():
        p.grad = None
    Xc = OrderedDict((k, v.cuda()) for k, v in X.items())
    logit = model.logits(Xc)
    logit.backward(g.cuda().view(-1, 1))
    torch.cuda.synchronize()
    return logit.detach()


def _run_cases(fm, D, cases, seed):
    """cases: (B, id dtype) pairs; each runs through FM(fused=True) and FM(fused=False) with the same weights."""
    fused = _model(fm, D, True, seed)
    plain = _model(fm, D, False, seed)
    plain.load_state_dict(fused.state_dict())
    for k, (B, dt) in enumerate(cases):
        X = _batch(fm, B, seed * 31 + k, dt)
        g = torch.randn(B, generator=torch.Generator().manual_seed(seed + k))
        for model, how in ((fused, "fused"), (plain, "layers")):
            logit = _step(model, X, g)
            check_against_restatement(model, fm, X, g, logit, "D%d %s %s B%d" % (D, how, str(dt)[6:], B))


@pytest.mark.parametrize("D", DIMS)
def test_fm_grid_of_dims_against_float64(D):
    """Tier-A tables of 2 (no id but 0 and 1), 3, 300 and 4000 rows (the last while the 1 M-float budget holds),
    tier-B tables of 5000, 70 000 (no padding row) and 1 000 000 rows, 13 numeric features, ~5 % padding ids;
    float64 and int64 id columns; 6181 samples (not a multiple of the 2048-sample tier-A block) and 1."""
    fm = _features(GRID_VOCABS, 13, no_pad=NO_PAD)
    _run_cases(fm, D, [(6181, torch.float64), (6181, torch.int64), (1, torch.float64), (1, torch.int64)], seed=D)


@pytest.mark.parametrize("D,n_num", [(40, 1), (44, 1), (16, 0), (10, 0), (24, 33), (7, 33)])
def test_fm_numeric_feature_counts_against_float64(D, n_num):
    """1 numeric feature at D = 40 / 44: fm_numeric_blocks_kernel at its LDS limit; none (bias only; every column an id:
    the forward's int64 instantiation); 33, more than kTaNumMax: fm_numeric_partial_kernel."""
    fm = _features([3, 300, 5000, 70000], n_num, no_pad=NO_PAD)
    _run_cases(fm, D, [(6181, torch.float64), (6181, torch.int64)], seed=1000 + D + n_num)


def test_fm_tier_a_budget_runs_out_against_float64():
    """Six 4000-row tables at D = 64: 65 x 4000 floats each, so four fit tier A's 1 M-float budget, two go to tier B."""
    fm = _features([4000] * 6 + [5000], 13)
    _run_cases(fm, 64, [(6181, torch.float64)], seed=64064)


@pytest.mark.parametrize("D", [65, 100, 260])
def test_fm_dims_the_fused_kernels_do_not_take(D):
    """FM(fused=True) at dims without a fused forward (65, 260; 100 is 25 float4s and fused) gives what fused=False
    gives, within the bound, and does not raise."""
    fm = _features([3, 300, 5000, 70000], 13, no_pad=NO_PAD)
    _run_cases(fm, D, [(6181, torch.float64), (1, torch.int64)], seed=2000 + D)


@pytest.mark.parametrize("D", [10, 16, 40])
def test_fm_table_read_by_two_fields_against_float64(D):
    """A tier-A table (300 rows) and a tier-B table (5000 rows) each read by two fields.  The embedding tables are shared,
    the LR layer's are not (the reference's LogisticRegression builds its own per feature): each LR table must get the
    gradient of its own field's lookups only."""
    fm = _features([3, 300, 5000, 70000], 13, shared=[1, 2], no_pad=NO_PAD)
    _run_cases(fm, D, [(6181, torch.float64), (1, torch.float64)], seed=3000 + D)


def _bench_case(D, seed, pad_frac=0.03):
    import bench
    fmw = bench.CriteoFeatureMap(D)
    batch = bench.synthetic_batch(65536, seed, "zipf", "cpu")
    gen = torch.Generator().manual_seed(seed)
    for name, spec in fmw.fm.features.items():
        if spec["type"] == "categorical":
            col = fmw.fm.get_column_index(name)
            batch[torch.rand(batch.shape[0], generator=gen) < pad_frac, col] = 0
    return fmw.fm, batch


@pytest.mark.parametrize("D,chain", [(16, "bce"), (10, "g")])
def test_bench_configuration_zipf_ids_against_float64(D, chain):
    """The bench's model and batch (26 Criteo-sized tables, 13 numeric features, B = 65 536, Zipf-like ids as float64
    columns of one batch tensor, 3 % of them the padding id) against the restatement.  D = 16 through the bench's
    sigmoid + BCE chain (g = dL/dlogit as the fused backward received it), D = 10 with a random g."""
    import bench
    from recbox_amd import ops
    from recbox_amd.ranking.pytorch.models import FM
    from recbox_amd.ranking.pytorch.torch_utils import get_loss
    torch.set_num_threads(min(16, torch.get_num_threads()))
    fm, batch = _bench_case(D, seed=7 + D)
    model = FM(fm, D, fused=True)
    bench.init_weights(model)
    model.cuda()
    batch = batch.cuda()
    X, y = bench.slice_inputs(fm, batch)
    if chain == "bce":
        logit, prob = model.logits(X, with_prob=True)
        seen = []
        logit.register_hook(lambda t: seen.append(t.detach().clone()))
        loss = get_loss("binary_crossentropy")(ops.sigmoid_output(logit, prob), y, reduction="mean")
        loss.backward()
        g = seen[0].view(-1)
    else:
        g = torch.randn(65536, generator=torch.Generator().manual_seed(D)).cuda()
        logit = model.logits(X)
        logit.backward(g.view(-1, 1))
    torch.cuda.synchronize()
    Xh = OrderedDict((k, v.cpu()) for k, v in X.items())
    check_against_restatement(model, fm, Xh, g, logit.detach(), "bench D%d zipf %s" % (D, chain))


@pytest.mark.parametrize("D", [16, 10])
def test_hot_id_long_chains_against_float64_and_repeatable(D):
    """B = 65 536, four fields over 10 000-row tables (tier B), 80 % of every field's lookups on one id: each hot row is a
    chain of ~3 300 chunks of the sorted reduce, which the long fix-up splits between several workgroups (KW > 1: partial
    slots, the arrival counter, its reset by the last workgroup) with FmPolicy's count and prefetched row.  Against the
    restatement, then a second backward over the same forward and sort (retain_graph): the gradients must come out exactly
    twice the first ones."""
    feats = OrderedDict()
    feats["I0"] = {"source": "", "type": "numeric"}
    for i in range(4):
        feats["H%d" % i] = {"source": "", "type": "categorical", "vocab_size": 10000, "padding_idx": 0}
    feats["C0"] = {"source": "", "type": "categorical", "vocab_size": 3, "padding_idx": 0}
    fm = _FM(feats)
    B = 65536
    cols = hot_id_batch(B, seed=D)
    X = OrderedDict()
    X["I0"] = torch.rand(B, generator=torch.Generator().manual_seed(D), dtype=torch.float64)
    for i, c in enumerate(cols):
        X["H%d" % i] = c.double()
    X["C0"] = torch.randint(0, 3, (B,), generator=torch.Generator().manual_seed(D + 1)).double()
    model = _model(fm, D, True, seed=D)
    g = torch.randn(B, generator=torch.Generator().manual_seed(5 + D))
    Xc = OrderedDict((k, v.cuda()) for k, v in X.items())
    for p in model.parameters():
        p.grad = None
    logit = model.logits(Xc)
    logit.backward(g.cuda().view(-1, 1), retain_graph=True)
    torch.cuda.synchronize()
    check_against_restatement(model, fm, X, g, logit.detach(), "hot D%d" % D)
    first = [p.grad.clone() for p in model.parameters()]
    logit.backward(g.cuda().view(-1, 1))
    torch.cuda.synchronize()
    for (n, p), g1 in zip(model.named_parameters(), first):
        assert torch.equal(p.grad, 2 * g1), "second backward over the same sort differs: " + n


@pytest.mark.xfail(strict=True, reason="the fused body refuses D > 128 (kFmMaxDim): with FmPolicy the sorted tier's 64-lane "
                                       "vector form leaves the embedding gradient of a table with two adjacent hot rows "
                                       "percent-level wrong; the shared kernels (test_gpu_embed_dims.py: GenericPolicy / "
                                       "DotPolicy hot rows at D = 132, 256), the forward and the count column are cleared, "
                                       "FmPolicy::flush's cnt * w_r term remains")
def test_fused_body_at_dim_132_with_hot_rows(monkeypatch):
    """ops.fm_fused itself at D = 132 (past the model's dim rule) with rows of thousands of lookups, against the
    restatement.  Today rbx_fm_fwd refuses the dim; before that refusal, the sorted tier's 64-lane vector form
    (segment_*_kernel<FmPolicy, 64, 1, true>) returned hot rows up to 2 % off.  The same kernels with GenericPolicy and
    DotPolicy meet the bound at D = 132 and 256 with far hotter rows (test_gpu_embed_dims.py), and with the refusal lifted
    only the 3-row table's embedding gradient fails here (its LR gradient, i.e. the count column, the 2-row and 5000-row
    tables and the logit pass): the defect is in FmPolicy::flush's - cnt * w_r term for adjacent hot rows of one table.
    Once that is fixed and the refusal lifted, this test passes and the xfail goes."""
    import recbox_amd.ranking.pytorch.layers.embeddings as E
    monkeypatch.setattr(E, "fm_fused_takes_dim", lambda dim: True)
    fm = _features([2, 3, 5000], 1)
    model = _model(fm, 132, True, seed=132)
    X = _batch(fm, 6181, 132, torch.float64)
    g = torch.randn(6181, generator=torch.Generator().manual_seed(132))
    logit = _step(model, X, g)
    check_against_restatement(model, fm, X, g, logit, "D132 fused body")
