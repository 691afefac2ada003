"""DIEN's attention-gated GRU without a GPU: the float64 restatement (tests/attgru64.py) against the reference fixture
tests/golden/dien.npz (recorded from the live reference by tests/gen_golden_dien.py) -- ``DynamicRNN`` and the two cells, outputs
and gradients; the RecBole mirrors (recbole.sequential, recbole.layers) on CPU tensors, loading the fixture's state_dicts with
``strict=True``, against its outputs and gradients at 1e-4; the compat paths; the C ABI's symbols."""
import pytest
import torch

import attgru64
from conftest import Fixture, assert_close

TOL = 1e-4
CELLS = {"agru": "AGRU", "augru": "AUGRU"}


def _dims(fx, c):
    return fx["in%d" % c]["keys"].shape


@pytest.mark.parametrize("c", [0, 1])
@pytest.mark.parametrize("tag", ["agru", "augru"])
def test_restatement_against_the_reference_cells(tag, c):
    fx = Fixture("dien")
    t = fx.tensors("in%d" % c)
    p = {k: v.double().requires_grad_() for k, v in fx.tensors("p%d_%s" % (c, tag)).items()}
    x, h, a = (v.double().requires_grad_() for v in (t["keys"][:, 0], t["h"], t["a"]))
    hy = attgru64.cell_step(CELLS[tag], x, h, a, p["weight_ih"], p["weight_hh"], p["bias_ih"], p["bias_hh"])
    (hy * t["up_vec"].double()).sum().backward()
    g = fx["g%d_%s" % (c, tag)]
    assert_close(hy, fx["out%d_%s" % (c, tag)]["hy"], TOL, "hy")
    for name, v in (("x", x), ("h", h), ("a", a)):
        assert_close(v.grad, g[name], TOL, "d" + name)
    for name, v in p.items():
        assert_close(v.grad, g[name], TOL, "grad " + name)
    if tag == "agru":
        H = h.shape[1]
        assert (p["weight_ih"].grad[H:2 * H] == 0).all() and (p["bias_hh"].grad[H:2 * H] == 0).all()


@pytest.mark.parametrize("c", [0, 1])
@pytest.mark.parametrize("tag", ["agru", "augru"])
def test_restatement_against_the_reference_dynamic_rnn(tag, c):
    fx = Fixture("dien")
    t = fx.tensors("in%d" % c)
    p = {k: v.double().requires_grad_() for k, v in fx.tensors("p%d_dyn_%s" % (c, tag)).items()}
    keys, att = t["keys"].double().requires_grad_(), t["att"].double().requires_grad_()
    out, h_n = attgru64.att_gru_layer(keys, att, p["rnn.weight_ih"], p["rnn.weight_hh"], p["rnn.bias_ih"], p["rnn.bias_hh"], None,
                                      t["lengths"], CELLS[tag])
    (out * t["up_seq"].double()).sum().backward()
    g = fx["g%d_dyn_%s" % (c, tag)]
    assert_close(out, fx["out%d_dyn_%s" % (c, tag)]["out"], TOL, "out")
    last = out[torch.arange(out.shape[0]), t["lengths"] - 1]
    assert torch.equal(h_n, last)                                         # h_n is the output at position lengths - 1
    assert_close(keys.grad, g["keys"], TOL, "dkeys")
    assert_close(att.grad, g["att"], TOL, "datt")
    for name, v in p.items():
        assert_close(v.grad, g[name], TOL, "grad " + name)
    # float32 run of the same restatement: what the fp32 bar of the GPU tests is made of
    out32, _ = attgru64.att_gru_layer(t["keys"], t["att"], *(p[k].detach().float() for k in ("rnn.weight_ih", "rnn.weight_hh",
                                                                                            "rnn.bias_ih", "rnn.bias_hh")),
                                      None, t["lengths"], CELLS[tag])
    assert out32.dtype == torch.float32
    assert_close(out32, out, 1e-5, "fp32 restatement")


def _check_module(fx, c, tag, module, run, inputs, device="cpu"):
    module.load_state_dict(fx.tensors("p%d_%s" % (c, tag)), strict=True)
    module = module.to(device)
    t = fx.tensors("in%d" % c, device=device)
    leaves = {k: t[k].clone().requires_grad_() for k in inputs}
    outs, loss = run(module, t, leaves)
    loss.backward()
    for name, v in outs.items():
        assert_close(v, fx["out%d_%s" % (c, tag)][name], TOL, "%s %s" % (tag, name))
    g = fx["g%d_%s" % (c, tag)]
    for name, v in leaves.items():
        assert_close(v.grad, g[name], TOL, "%s d%s" % (tag, name))
    for name, p in module.named_parameters():
        got = p.grad if p.grad is not None else torch.zeros_like(p)
        assert_close(got, g[name], TOL, "%s grad %s" % (tag, name))


def run_cell(m, t, v):
    hy = m(v["x"], v["h"], v["a"])
    return {"hy": hy}, (hy * t["up_vec"]).sum()


def run_dynamic_packed(m, t, v):
    from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence
    L = v["keys"].shape[1]
    lengths = t["lengths"].cpu()
    pk = pack_padded_sequence(v["keys"], lengths=lengths, batch_first=True, enforce_sorted=False)
    pa = pack_padded_sequence(v["att"], lengths=lengths, batch_first=True, enforce_sorted=False)
    y, _ = pad_packed_sequence(m(pk, pa), batch_first=True, padding_value=0.0, total_length=L)
    return {"out": y}, (y * t["up_seq"]).sum()


def run_dynamic_padded(m, t, v):
    y, h_n = m.forward_padded(v["keys"], v["att"], t["lengths"])
    return {"out": y}, (y * t["up_seq"]).sum()


def run_evolving(m, t, v):
    y = m(v["queries"], v["keys"], t["lengths"])
    return {"y": y}, (y * t["up_vec"]).sum()


def run_extractor(m, t, v):
    rnn, aux = m(v["keys"], t["lengths"], v["neg"])
    return {"rnn": rnn, "aux": aux}, (rnn * t["up_seq"]).sum() + aux


def build(fx, c, tag):
    """(module, run, names of the input leaves) of a fixture tag."""
    from recbox_amd.recbole import sequential as S
    B, L, E = _dims(fx, c)
    if tag in CELLS:
        return (S.AGRUCell if tag == "agru" else S.AUGRUCell)(E, E), run_cell, ("h", "a")
    if tag.startswith("dyn_"):
        return S.DynamicRNN(E, E, gru=CELLS[tag[4:]]), None, ("keys", "att")
    if tag.startswith("evo_"):
        return (S.InterestEvolvingLayer(torch.arange(L).view(1, -1), E, E, [4 * E, 16, 8], gru=tag[4:]), run_evolving,
                ("queries", "keys"))
    return S.InterestExtractorNetwork(E, E, [2 * E, 16, 1]), run_extractor, ("keys", "neg")


@pytest.mark.parametrize("c", [0, 1])
@pytest.mark.parametrize("tag", ["agru", "augru"])
def test_cell_mirrors_against_the_reference_fixture(tag, c):
    fx = Fixture("dien")
    m, _, _ = build(fx, c, tag)
    assert list(m.state_dict().keys()) == ["weight_ih", "weight_hh", "bias_ih", "bias_hh"]
    m.load_state_dict(fx.tensors("p%d_%s" % (c, tag)), strict=True)
    t = fx.tensors("in%d" % c)
    x, h, a = (v.clone().requires_grad_() for v in (t["keys"][:, 0], t["h"], t["a"]))
    hy = m(x, h, a)
    (hy * t["up_vec"]).sum().backward()
    g = fx["g%d_%s" % (c, tag)]
    assert_close(hy, fx["out%d_%s" % (c, tag)]["hy"], TOL, "hy")
    for name, v in (("x", x), ("h", h), ("a", a)):
        assert_close(v.grad, g[name], TOL, "d" + name)
    for name, p in m.named_parameters():
        assert_close(p.grad, g[name], TOL, "grad " + name)


@pytest.mark.parametrize("c", [0, 1])
@pytest.mark.parametrize("form", ["packed", "padded"])
@pytest.mark.parametrize("tag", ["dyn_agru", "dyn_augru"])
def test_dynamic_rnn_mirror_against_the_reference_fixture(tag, form, c):
    fx = Fixture("dien")
    m, _, inputs = build(fx, c, tag)
    _check_module(fx, c, tag, m, run_dynamic_packed if form == "packed" else run_dynamic_padded, inputs)


@pytest.mark.parametrize("c", [0, 1])
@pytest.mark.parametrize("tag", ["evo_GRU", "evo_AIGRU", "evo_AGRU", "evo_AUGRU", "ext"])
def test_layer_mirrors_against_the_reference_fixture(tag, c):
    fx = Fixture("dien")
    m, run, inputs = build(fx, c, tag)
    _check_module(fx, c, tag, m, run, inputs)


def test_dynamic_rnn_refuses_unpacked_input_and_keeps_the_packing():
    from torch.nn.utils.rnn import pack_padded_sequence
    from recbox_amd.recbole.sequential import DynamicRNN
    m = DynamicRNN(4, 4, gru="AUGRU")
    with pytest.raises(NotImplementedError):
        m(torch.zeros(3, 2, 4), torch.zeros(3, 2))
    lengths = torch.tensor([1, 3, 2])
    pk = pack_padded_sequence(torch.randn(3, 3, 4), lengths, batch_first=True, enforce_sorted=False)
    pa = pack_padded_sequence(torch.rand(3, 3), lengths, batch_first=True, enforce_sorted=False)
    y = m(pk, pa)
    assert torch.equal(y.batch_sizes, pk.batch_sizes) and torch.equal(y.sorted_indices, pk.sorted_indices)
    assert torch.equal(y.unsorted_indices, pk.unsorted_indices)


def test_layers_of_recbole():
    from recbox_amd.recbole import layers as L
    m = L.MLPLayers([8, 6, 3], dropout=0.1, activation="Dice", bn=True)
    assert [type(x).__name__ for x in m.mlp_layers] == ["Dropout", "Linear", "BatchNorm1d", "Dice"] * 2
    assert "mlp_layers.1.weight" in m.state_dict() and not any("alpha" in k for k in m.state_dict())
    assert not list(L.Dice(3).parameters())
    assert L.activation_layer("none") is None and L.activation_layer(None) is None
    assert isinstance(L.activation_layer("leakyrelu"), torch.nn.LeakyReLU) and isinstance(L.activation_layer(torch.nn.ReLU),
                                                                                           torch.nn.ReLU)
    s = torch.randn(5, 3)
    assert_close(L.Dice(3)(s), torch.sigmoid(s) * s, 1e-7, "Dice")
    att = L.SequenceAttLayer(None, [16, 8, 4], "sigmoid", softmax_stag=True, return_seq_weight=True)
    w = att(torch.randn(5, 4), torch.randn(5, 6, 4), torch.tensor([1, 6, 3, 2, 5]))
    assert tuple(w.shape) == (5, 1, 6) and (w[0, 0, 1:] == 0).all()
    assert_close(w.sum(dim=2), torch.ones(5, 1), 1e-6, "softmax rows")
    zero_fill = L.SequenceAttLayer(None, [16, 8, 4], "sigmoid", softmax_stag=False, return_seq_weight=False)
    assert tuple(zero_fill(torch.randn(5, 4), torch.randn(5, 6, 4), torch.tensor([1, 6, 3, 2, 5])).shape) == (5, 1, 4)


def test_the_op_refuses_cpu_tensors():
    from recbox_amd import ops
    x, att = torch.randn(3, 2, 4), torch.rand(3, 2)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.att_gru(x, att, torch.randn(12, 4), torch.randn(12, 4))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.att_gru_torch(x, att, torch.randn(12, 4), torch.randn(12, 4))
    assert ops.config.attgru_fused is True


def test_supported_shapes_and_symbols():
    from recbox_amd import _lib, ops
    for name in ("rbx_attgru_supported", "rbx_attgru_fwd", "rbx_attgru_bwd"):
        assert hasattr(_lib.lib, name)
    for cell in ("AGRU", "AUGRU"):
        assert ops.att_gru_supported(4, 1, cell) and ops.att_gru_supported(128, 50, cell) and ops.att_gru_supported(100, 20, cell)
        assert not ops.att_gru_supported(6, 7, cell) and not ops.att_gru_supported(132, 7, cell)
        assert not ops.att_gru_supported(0, 7, cell) and not ops.att_gru_supported(16, 0, cell)
    assert not _lib.lib.rbx_attgru_supported(16, 7, 2) and not _lib.lib.rbx_attgru_supported(16, 7, -1)
    with pytest.raises(ValueError):
        ops.att_gru_supported(16, 7, "GRU")


def test_rechub_dien_on_cpu_tensors():
    from test_gpu_attgru import dien_model_and_batch
    for kind in ("GRU", "AIGRU", "AGRU", "AUGRU"):
        model, x = dien_model_and_batch(kind)
        y, aux = model(x)
        assert tuple(y.shape) == (x["item"].shape[0],) and aux.dim() == 0
        (torch.nn.functional.binary_cross_entropy(y, x["label"]) + model.alpha * aux).backward()
        grads = {n: p.grad for n, p in model.named_parameters()}
        assert all(g is None or torch.isfinite(g).all() for g in grads.values())
        assert all(grads[n] is not None and (grads[n] != 0).any() for n in grads
                   if n.startswith("interest_evolution.dynamic_rnn.") and "weight" in n)
    keys = [k for k in model.state_dict() if k.startswith("interest_evolution.")]
    assert "interest_evolution.dynamic_rnn.rnn.weight_ih" in keys
    assert "interest_evolution.attention_layer.att_mlp_layers.mlp_layers.1.weight" in keys
    assert "interest_extractor.gru.weight_ih_l0" in model.state_dict()


def test_compat_resolves_dien_to_the_mirror():
    import importlib
    from recbox_amd import compat
    from recbox_amd.rechub.models import ranking
    assert all("DIEN" in names for path, names in compat.alias_also().items() if path.endswith(".models.ranking"))
    report = compat.install(prefixes=("torch_rechub", "recbox"), overlay=False)
    try:
        for root in ("torch_rechub", "recbox.third_party.rechub"):
            assert importlib.import_module(root + ".models.ranking").DIEN is ranking.DIEN
    finally:
        compat.uninstall(report)
