"""The fused attention-gated GRU on the HIP path (csrc/rbx_gru.hip: ops.att_gru, the RecBole DIEN mirrors, rechub's DIEN)
against the restatement of tests/attgru64.py in float64 on the CPU, under the scale-aware bar of tests/fp32_bar.py: per tensor
max|got - want| <= max(4 e32, 2e-6 max|want|), e32 the error of the float32 CPU run of the same restatement (nothing the
kernels produce enters the bar; factor 4 everywhere but for one result of the DIEN step, see DIEN_FACTORS).  Every float64 comparison also runs the fp32 step-loop composition
(ops.att_gru_torch) on the GPU through the same asserts.  Inputs: x ~ N(0, 1), weights and biases ~ U(-1/sqrt(H), 1/sqrt(H)),
att ~ U(0, 1), lengths uniform in 0..L, upstream gradients on out and h_n ~ N(0, 1) / sqrt(B L)."""
import pytest
import torch

import attgru64
from conftest import Fixture
from fp32_bar import FACTOR, assert_bar, report

pytestmark = pytest.mark.gpu
CELLS = ("AGRU", "AUGRU")
# (L, I, H): one step; H = 16 (one wavefront); H = 64 (four); H = 100 (seven wavefronts, the last one a quarter full: the d_att
# sum must skip lanes; I = 50 is no multiple of 4); H = 20 (a partial second wavefront); H = 4 (the floor); H = 128 (the top:
# eight wavefronts, the 32-k-step register layout); H = 96
SHAPES = [(1, 16, 16), (7, 16, 16), (50, 64, 64), (20, 50, 100), (33, 20, 20), (9, 8, 4), (50, 128, 128), (12, 32, 96)]
BATCHES = [37, 301]
NAMES = ("out", "h_n", "dx", "datt", "dW_ih", "dW_hh", "db_ih", "db_hh", "dh0")


def _inputs(B, L, I, H, seed=0):
    g = torch.Generator().manual_seed(100000 * L + 1000 * I + 10 * H + B + seed)
    bound = 1.0 / H ** 0.5

    def uni(*shape):
        return (torch.rand(*shape, generator=g) * 2 - 1) * bound
    return {"x": torch.randn(B, L, I, generator=g), "params": [uni(3 * H, I), uni(3 * H, H), uni(3 * H), uni(3 * H)],
            "h0": torch.randn(B, H, generator=g), "att": torch.rand(B, L, generator=g),
            "lengths": torch.randint(0, L + 1, (B,), generator=g),
            "up_out": torch.randn(B, L, H, generator=g) / (B * L) ** 0.5,
            "up_hn": torch.randn(B, H, generator=g) / (B * L) ** 0.5}


def _fused(x, att, p, h0, lengths, cell):
    from recbox_amd import ops
    return ops.att_gru(x, att, p[0], p[1], p[2], p[3], h0, lengths, cell)


def _composition(x, att, p, h0, lengths, cell):
    from recbox_amd import ops
    return ops.att_gru_torch(x, att, p[0], p[1], p[2], p[3], h0, lengths, cell)


def _restatement(x, att, p, h0, lengths, cell):
    return attgru64.att_gru_layer(x, att, p[0], p[1], p[2], p[3], h0, lengths, cell)


def _run(fn, inp, cell, device, dtype, bias=True, h0=True, lengths=True, use=("out", "h_n")):
    """One layer through ``fn``; returns the tensors of NAMES (None where a form has none)."""
    def leaf(t):
        return t.detach().to(device=device, dtype=dtype).requires_grad_(True)
    x, att = leaf(inp["x"]), leaf(inp["att"])
    p = [leaf(t) if (i < 2 or bias) else None for i, t in enumerate(inp["params"])]
    h0s = leaf(inp["h0"]) if h0 else None
    lens = inp["lengths"].to(device) if lengths else None
    out, hn = fn(x, att, p, h0s, lens, cell)
    loss = 0
    if "out" in use:
        loss = loss + (out * inp["up_out"].to(device=device, dtype=out.dtype)).sum()
    if "h_n" in use:
        loss = loss + (hn * inp["up_hn"].to(device=device, dtype=hn.dtype)).sum()
    loss.backward()
    return ([out.detach(), hn.detach(), x.grad, att.grad] + [t.grad if t is not None else None for t in p]
            + [h0s.grad if h0s is not None else None])


def _compare(inp, cell, tag, fns=(("composition", _composition), ("fused", _fused)), **form):
    want = _run(_restatement, inp, cell, "cpu", torch.float64, **form)
    ref32 = _run(_restatement, inp, cell, "cpu", torch.float32, **form)
    for name, fn in fns:
        got = _run(fn, inp, cell, "cuda", torch.float32, **form)
        for what, a, b, c in zip(NAMES, got, want, ref32):
            assert (a is None) == (b is None), "%s %s %s" % (name, what, tag)
            if b is not None:
                assert_bar("%s_%s %s %s" % (name, what, cell, tag), a, b, c)
    report("attgru %s %s" % (cell, tag))


@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("L,I,H", SHAPES)
def test_against_float64(L, I, H, B, cell):
    """Bias, h0 and lengths all given."""
    from recbox_amd import ops
    assert ops.att_gru_supported(H, L, cell)                   # the whole list is inside the shipped range (4 .. 128)
    _compare(_inputs(B, L, I, H), cell, "B=%d L=%d I=%d H=%d" % (B, L, I, H))


def test_fused_op_runs_the_kernels(monkeypatch):
    """``ops.att_gru`` on a supported shape enters rbx_attgru_fwd / rbx_attgru_bwd; with the switch off, at H = 6, for a strided
    view or for float64 it does not."""
    from recbox_amd import ops
    calls = []
    real = ops.lib

    class Spy(object):
        def rbx_attgru_fwd(self, *a):
            calls.append("fwd")
            return real.rbx_attgru_fwd(*a)

        def rbx_attgru_bwd(self, *a):
            calls.append("bwd")
            return real.rbx_attgru_bwd(*a)

        def __getattr__(self, name):
            return getattr(real, name)
    monkeypatch.setattr(ops, "lib", Spy())
    inp = _inputs(37, 7, 16, 16, seed=1)
    for cell in CELLS:
        _run(_fused, inp, cell, "cuda", torch.float32)
    assert calls == ["fwd", "bwd"] * 2
    monkeypatch.setattr(ops.config, "attgru_fused", False)
    _run(_fused, inp, "AUGRU", "cuda", torch.float32)
    assert len(calls) == 4
    monkeypatch.setattr(ops.config, "attgru_fused", True)
    assert not ops.att_gru_supported(6, 7)
    _compare(_inputs(37, 7, 10, 6, seed=1), "AUGRU", "refused H=6", fns=(("refused", _fused),))
    x, att = inp["x"].cuda(), inp["att"].cuda()
    p = [t.cuda() for t in inp["params"]]
    view = torch.randn(37, 7, 32, device="cuda")[:, :, :16]                   # an oddly strided view: the composition
    ops.att_gru(view, att, p[0], p[1])
    ops.att_gru(x.double(), att.double(), p[0], p[1])                         # float64: the composition
    assert len(calls) == 4
    out, _ = ops.att_gru(x, att.view(37, 7, 1), p[0], p[1])                   # [B, L, 1] and [B, 1, L] scores are reshaped
    out2, _ = ops.att_gru(x, att.view(37, 1, 7), p[0], p[1])
    assert len(calls) == 6 and torch.equal(out, out2)


@pytest.mark.parametrize("cell", CELLS)
def test_single_sample(cell):
    _compare(_inputs(1, 7, 16, 16, seed=2), cell, "B=1")
    _compare(_inputs(1, 20, 50, 100, seed=2), cell, "B=1 H=100")


@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("h0", [True, False])
@pytest.mark.parametrize("lengths", [True, False])
def test_forms(bias, h0, lengths, cell):
    _compare(_inputs(37, 7, 16, 16, seed=3), cell, "bias=%s h0=%s lengths=%s" % (bias, h0, lengths), bias=bias, h0=h0,
             lengths=lengths)
    _compare(_inputs(37, 20, 50, 100, seed=3), cell, "H=100 bias=%s h0=%s lengths=%s" % (bias, h0, lengths), bias=bias, h0=h0,
             lengths=lengths)


@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("use", [("h_n",), ("out",)])
def test_only_one_output_used(use, cell):
    """DIEN reads h_n alone, a sequence model out alone: the unused output's gradient is absent, not a zero tensor."""
    _compare(_inputs(37, 7, 16, 16, seed=4), cell, "use=%s" % (use,), use=use)
    _compare(_inputs(301, 50, 64, 64, seed=4), cell, "use=%s H=64" % (use,), use=use, bias=False, h0=False, lengths=False)


@pytest.mark.parametrize("cell", CELLS)
def test_all_lengths_zero(cell):
    inp = _inputs(37, 7, 16, 16, seed=6)
    inp["lengths"] = torch.zeros(37, dtype=torch.long)
    _compare(inp, cell, "lengths all 0")
    got = _run(_fused, inp, cell, "cuda", torch.float32)
    assert (got[0] == 0).all() and torch.equal(got[1].cpu(), inp["h0"]) and (got[2] == 0).all() and (got[3] == 0).all()
    assert torch.equal(got[8].cpu(), inp["up_hn"])            # dh0 = the upstream gradient of h_n, passed through unchanged


@pytest.mark.parametrize("cell", CELLS)
def test_lengths_0_1_and_L_share_a_tile(cell):
    inp = _inputs(37, 9, 16, 20, seed=7)
    inp["lengths"] = torch.tensor(([0, 1, 9, 1, 0, 9, 9, 0, 1, 4] * 4)[:37])
    assert set(inp["lengths"][:16].tolist()) >= {0, 1, 9}    # one workgroup's 16 samples mix all three
    _compare(inp, cell, "lengths 0 / 1 / L in one tile")
    inp["lengths"] = inp["lengths"].int()                     # int32 lengths read the same
    _compare(inp, cell, "int32 lengths", fns=(("fused", _fused),))


@pytest.mark.parametrize("cell", CELLS)
def test_masked_positions_are_exactly_zero(cell):
    inp = _inputs(301, 33, 20, 20, seed=8)
    got = _run(_fused, inp, cell, "cuda", torch.float32)
    dead = (torch.arange(33).unsqueeze(0) >= inp["lengths"].unsqueeze(1)).cuda()
    assert dead.any() and (~dead).any()
    for k in (0, 2, 3):                                                       # out, dx (d_gi's effect), d_att
        assert (got[k][dead] == 0).all() and (got[k][~dead] != 0).any(), NAMES[k]


@pytest.mark.parametrize("cell", CELLS)
def test_scores_from_a_softmax_over_the_valid_positions(cell):
    """DIEN's own form: zeros beyond the length, a distribution over the positions before it."""
    inp = _inputs(37, 20, 50, 100, seed=11)
    L = 20
    inp["lengths"] = inp["lengths"].clamp(min=1)
    valid = torch.arange(L).unsqueeze(0) < inp["lengths"].unsqueeze(1)
    logits = (inp["att"] * 6 - 3).masked_fill(~valid, float("-inf"))
    inp["att"] = torch.softmax(logits, dim=1)
    _compare(inp, cell, "softmax scores")


@pytest.mark.parametrize("cell", CELLS)
def test_scores_outside_the_unit_interval(cell):
    """No clamp: negative scores and scores above 1 are taken as written."""
    inp = _inputs(37, 7, 16, 20, seed=12)
    inp["att"] = inp["att"] * 3 - 1                                           # U(-1, 2)
    assert (inp["att"] < 0).any() and (inp["att"] > 1).any()
    _compare(inp, cell, "scores in (-1, 2)")


def test_agru_leaves_the_update_rows_without_gradient():
    for L, I, H in ((7, 16, 16), (20, 50, 100)):
        got = _run(_fused, _inputs(37, L, I, H, seed=13), "AGRU", "cuda", torch.float32)
        for k in (4, 5, 6, 7):                                                # dW_ih, dW_hh, db_ih, db_hh
            assert (got[k][H:2 * H] == 0).all(), NAMES[k]
            assert (got[k][:H] != 0).any() and (got[k][2 * H:] != 0).any(), NAMES[k]


@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("L,I,H", [(50, 64, 64), (20, 50, 100), (50, 128, 128)])
def test_determinism(L, I, H, cell):
    inp = _inputs(301, L, I, H, seed=9)
    first = _run(_fused, inp, cell, "cuda", torch.float32)
    second = _run(_fused, inp, cell, "cuda", torch.float32)
    for what, a, b in zip(NAMES, first, second):
        assert torch.equal(a, b), what


def _capture(step, zero_grads):
    """Warm up on a side stream, capture ``step`` with torch.cuda.graph on one stream; returns (graph, what step returned)."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    zero_grads()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    return graph, out


def test_graph_capture_replays_the_eager_bits():
    from recbox_amd import ops
    B, L, I, H = 301, 20, 50, 100
    inp = _inputs(B, L, I, H, seed=10)
    eager = _run(_fused, inp, "AUGRU", "cuda", torch.float32)
    xs = torch.zeros(B, L, I, device="cuda").requires_grad_(True)
    atts = torch.full((B, L), 0.5, device="cuda").requires_grad_(True)
    ps = [p.cuda().requires_grad_(True) for p in inp["params"]]
    h0 = inp["h0"].cuda().requires_grad_(True)
    lens = torch.full((B,), L, device="cuda")
    uo, uh = inp["up_out"].cuda(), inp["up_hn"].cuda()

    def step():
        out, hn = ops.att_gru(xs, atts, ps[0], ps[1], ps[2], ps[3], h0, lens, "AUGRU")
        ((out * uo).sum() + (hn * uh).sum()).backward()
        return out, hn

    def zero():
        for t in [xs, atts, h0] + ps:
            t.grad = None
    graph, (out, hn) = _capture(step, zero)
    with torch.no_grad():
        xs.copy_(inp["x"].cuda())
        atts.copy_(inp["att"].cuda())
        lens.copy_(inp["lengths"].cuda())
    graph.replay()
    torch.cuda.synchronize()
    got = [out.detach(), hn.detach(), xs.grad, atts.grad] + [p.grad for p in ps] + [h0.grad]
    for what, a, b in zip(NAMES, got, eager):
        assert torch.equal(a, b), what


# ---- mirrors and model ------------------------------------------------------------------------------------------------------
TAGS = ["dyn_agru", "dyn_augru", "evo_GRU", "evo_AIGRU", "evo_AGRU", "evo_AUGRU", "ext"]


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("c", [0, 1])
@pytest.mark.parametrize("tag", TAGS)
def test_mirrors_match_the_reference_fixture(tag, c, fused, monkeypatch):
    """The RecBole mirrors on the GPU against tests/golden/dien.npz at the project's fixture tolerance (1e-4)."""
    import test_attgru_host as host
    from recbox_amd import ops
    monkeypatch.setattr(ops.config, "attgru_fused", fused)
    monkeypatch.setattr(ops.config, "gru_fused", fused)
    fx = Fixture("dien")
    m, run, inputs = host.build(fx, c, tag)
    if tag.startswith("dyn_"):
        host._check_module(fx, c, tag, m, host.run_dynamic_padded, inputs, device="cuda")
        m, _, _ = host.build(fx, c, tag)
        run = host.run_dynamic_packed
    host._check_module(fx, c, tag, m, run, inputs, device="cuda")


def dien_model_and_batch(kind, B=64, L=6, seed=0):
    """A small rechub-style DIEN (two history features of width 4: E = 8) and a batch of left-aligned histories with lengths
    in 1 .. L, on the CPU."""
    from recbox_amd.rechub.basic.features import SequenceFeature, SparseFeature
    from recbox_amd.rechub.models.ranking import DIEN
    torch.manual_seed(seed)
    profile = [SparseFeature("user", 11, 4)]
    target = [SparseFeature("item", 30, 4), SparseFeature("cate", 9, 4)]
    hist = [SequenceFeature("hist_item", 30, 4, pooling="concat", shared_with="item"),
            SequenceFeature("hist_cate", 9, 4, pooling="concat", shared_with="cate")]
    neg = [SequenceFeature("neg_item", 30, 4, pooling="concat", shared_with="item"),
           SequenceFeature("neg_cate", 9, 4, pooling="concat", shared_with="cate")]
    model = DIEN(profile, hist, neg, target, {"dims": [16, 8]}, {"dims": [16, 8]}, gru_type=kind, alpha=0.5)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() > 1:
                p.copy_(torch.randn(p.shape, generator=g) * 0.3)
    lengths = torch.randint(1, L + 1, (B,), generator=g)
    lengths[0], lengths[1] = 1, L
    valid = torch.arange(L).unsqueeze(0) < lengths.unsqueeze(1)
    x = {"user": torch.randint(0, 11, (B,), generator=g), "item": torch.randint(1, 30, (B,), generator=g),
         "cate": torch.randint(1, 9, (B,), generator=g), "label": (torch.rand(B, generator=g) < 0.4).float()}
    for name, V in (("hist_item", 30), ("hist_cate", 9), ("neg_item", 30), ("neg_cate", 9)):
        x[name] = torch.randint(1, V, (B, L), generator=g) * valid
    return model, x


def _dien_step(model, x):
    y, aux = model(x)
    (torch.nn.functional.binary_cross_entropy(y, x["label"].to(y.dtype)) + model.alpha * aux).backward()
    return y, aux


def _dien_results(model, x):
    y, aux = _dien_step(model, x)
    return [("y", y.detach()), ("aux", aux.detach())] + [(n, p.grad) for n, p in model.named_parameters() if p.grad is not None]


# a result of the DIEN step that needs another factor than 4: measured on the composition, see the test's docstring
DIEN_FACTORS = {"mlp.mlp.2.alpha": 8.0}


@pytest.mark.parametrize("kind", ["AGRU", "AUGRU"])
def test_dien_step_fused_and_unfused_against_float64(kind, monkeypatch):
    """One training step of the rechub-style DIEN: the model in float64 on the CPU (the mirrors' ATen branch) is the reference,
    its float32 CPU run gives the bar, and the GPU step with the fused recurrence and with the switch off are both held to it,
    every output and every parameter gradient.  The factor is 4 except for the one result of DIEN_FACTORS.

    Measured on the MI355X at factor 4, worst err / bar: AGRU 0.75 on both routes; AUGRU 0.55 fused and, for every tensor but
    one, 0.57 with the switch off.  The one: the gradient of ``mlp.mlp.2.alpha`` (the first Dice of the final MLP, 16 values,
    each a sum of 64 cancelling terms behind a BatchNorm), where the composition itself (switch off: ops.att_gru_torch, no
    kernel of csrc/rbx_gru.hip runs) has err 1.819e-08 against 4 e32 = 1.687e-08, 1.08 of the bar; e32 is 4.217e-09 there
    and 1.835e-08 for the same tensor under AGRU, so the float32 CPU run happened to land close.  The composition's own ratio
    sets the factor for that result: 8, the next power of two, at which the composition has 0.54 and the fused route 0.07."""
    from recbox_amd import ops
    model, x = dien_model_and_batch(kind)
    state = {k: v.clone() for k, v in model.state_dict().items()}
    ref32 = dict(_dien_results(model.train(), x))
    model64, _ = dien_model_and_batch(kind)
    model64.load_state_dict(state)
    want = dict(_dien_results(model64.double().train(), x))
    for fused in (True, False):
        monkeypatch.setattr(ops.config, "attgru_fused", fused)
        dut, _ = dien_model_and_batch(kind)
        dut.load_state_dict(state)
        got = dict(_dien_results(dut.cuda().train(), {k: v.cuda() for k, v in x.items()}))
        assert set(got) == set(want)
        for name in want:
            assert_bar("dien_%s %s fused=%s" % (name, kind, fused), got[name], want[name], ref32[name],
                       DIEN_FACTORS.get(name, FACTOR))
    report("attgru DIEN %s" % kind)


def test_dien_step_is_capturable_and_replays_the_eager_bits(monkeypatch):
    """DIEN's forward + backward as one graph: the lengths are counted on the device, nothing is packed or copied to the host
    (dien.py:209, 336 cannot be captured)."""
    from recbox_amd import ops
    monkeypatch.setattr(ops.config, "check_ids", False)      # the id check of the lookup reads a status word on the host
    ref, x = dien_model_and_batch("AUGRU")
    state = {k: v.clone() for k, v in ref.state_dict().items()}
    x = {k: v.cuda() for k, v in x.items()}

    def make():
        m, _ = dien_model_and_batch("AUGRU")
        m.load_state_dict(state)
        return m.cuda().train()
    eager = make()
    y_e, aux_e = _dien_step(eager, x)
    model = make()
    bufs = {k: (torch.ones_like(v) if v.dtype == torch.long else v.clone()) for k, v in x.items()}

    def step():
        return _dien_step(model, bufs)

    def zero():
        for p in model.parameters():
            p.grad = None
    graph, (y, aux) = _capture(step, zero)
    for k, v in x.items():
        bufs[k].copy_(v)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y.detach(), y_e.detach()) and torch.equal(aux.detach(), aux_e.detach())
    for (n, a), (_, b) in zip(model.named_parameters(), eager.named_parameters()):
        assert (a.grad is None) == (b.grad is None), n
        if a.grad is not None:
            assert torch.equal(a.grad, b.grad), n


def test_compat_resolves_dien_to_the_mirror():
    import importlib
    from recbox_amd import compat
    from recbox_amd.rechub.models import ranking
    report_ = compat.install(prefixes=("torch_rechub",))
    try:
        assert importlib.import_module("torch_rechub.models.ranking").DIEN is ranking.DIEN
    finally:
        compat.uninstall(report_)
