"""Self-attentive multi-interest pooling (``ops.sa_pool``), the parts that need no GPU: ComirecSA and SINE on the CPU path
against the live reference's fixture (tests/golden/rechub_multi_interest_sa.npz, written by tests/gen_golden_sa.py), their
state_dict keys, the compat entries, the einsum composition against the float64 restatement of tests/sa64.py, and MIND /
ComirecDR still loading their fixture by name after the base was factored."""
import importlib

import pytest
import torch

import sa64
from conftest import Fixture, assert_close, assert_grads_close

B, L, D, K, N_NEG = 16, 6, 8, 3, 3


def build(tag):
    from recbox_amd.rechub.basic.features import SequenceFeature, SparseFeature
    from recbox_amd.rechub.models.matching import SINE, ComirecSA
    if tag == "sine":
        return SINE(["hist_item_id"], ["item_id"], ["neg_items"], 23, D, 12, 5, K, L, num_heads=1)
    user = [SparseFeature("user_id", vocab_size=11, embed_dim=D)]
    hist = [SequenceFeature("hist_item_id", vocab_size=23, embed_dim=D, pooling="concat", shared_with="item_id")]
    item = [SparseFeature("item_id", vocab_size=23, embed_dim=D)]
    neg = [SequenceFeature("neg_items", vocab_size=23, embed_dim=D, pooling="concat", shared_with="item_id")]
    return ComirecSA(user, hist, item, neg, interest_num=K)


def check_model_against_fixture(tag, device):
    fx = Fixture("rechub_multi_interest_sa")
    model = build(tag)
    model.load_state_dict(fx.tensors("p_" + tag), strict=True)
    model = model.to(device).train()
    x = fx.tensors("in", device)
    for mode in ("user", "item"):
        model.mode = mode
        assert_close(model(x), fx["out_" + tag][mode], 1e-4, "%s mode=%s" % (tag, mode))
    model.mode = None
    y = model(x)
    assert_close(y, fx["out_" + tag]["y"], 1e-4, tag + " y")
    y.sum().backward()
    assert_grads_close(model, fx["g_" + tag], 1e-4)
    return model


@pytest.mark.parametrize("tag", ["comirec_sa", "sine"])
def test_models_match_the_reference_on_the_cpu_path(tag):
    fx = Fixture("rechub_multi_interest_sa")
    assert (fx["in"]["hist_item_id"] == 0).all(axis=1).sum() >= 2              # empty histories are in the fixture
    model = check_model_against_fixture(tag, "cpu")
    if tag == "comirec_sa":
        g3 = model.multi_interest_sa.W3.grad                                    # W3 is never read: no gradient, or zeros
        assert g3 is None or float(g3.abs().max()) == 0.0


@pytest.mark.parametrize("tag", ["comirec_sa", "sine"])
def test_state_dict_keys_equal_the_fixture(tag):
    fx = Fixture("rechub_multi_interest_sa")
    model = build(tag)
    assert set(model.state_dict().keys()) == set(fx["p_" + tag].keys())
    for k, v in model.state_dict().items():
        assert tuple(v.shape) == tuple(fx["p_" + tag][k].shape), k


def test_layer_parameters_and_hidden_dim():
    from recbox_amd.rechub.basic.layers import MultiInterestSA
    sa = MultiInterestSA(8, 3)
    assert [(n, tuple(p.shape)) for n, p in sa.named_parameters()] == [("W1", (8, 32)), ("W2", (32, 3)), ("W3", (8, 8))]
    assert all(0.0 <= float(p.detach().min()) and float(p.detach().max()) < 1.0 for p in sa.parameters())      # torch.rand
    sa = MultiInterestSA(8, 3, hidden_dim=12)                                                 # honoured: a superset
    assert sa.hidden_dim == 12 and tuple(sa.W1.shape) == (8, 12) and tuple(sa.W2.shape) == (12, 3)
    x = torch.randn(4, 5, 8)
    m = torch.tensor([[1, 1, 1, 0, 0]] * 4)
    assert torch.equal(sa(x, m), sa(x, m.unsqueeze(-1).float())) and tuple(sa(x, None).shape) == (4, 3, 8)


def test_compat_entries_and_paths():
    from recbox_amd import compat
    table = compat.alias_table()
    for root in ("torch_rechub", "recbox.third_party.rechub"):
        assert {"ComirecSA", "SINE"} <= set(table[root + ".models.matching"][1])
        assert table[root + ".models.matching.sine"] == ("recbox_amd.rechub.models.matching", ["SINE"])
        assert "ComirecSA" in table[root + ".models.matching.comirec"][1] + compat.alias_also()[root + ".models.matching.comirec"]
        assert table[root + ".basic.layers"] == ("recbox_amd.rechub.basic.layers", None)
    report = compat.install(prefixes=("torch_rechub",), overlay=False)
    try:
        from recbox_amd.rechub.basic import layers as ours
        from recbox_amd.rechub.models import matching
        for path, name in (("torch_rechub.models.matching.comirec", "ComirecSA"), ("torch_rechub.models.matching.sine", "SINE"),
                           ("torch_rechub.models.matching.comirec", "ComirecDR")):
            mod = importlib.import_module(path)
            if getattr(mod, "__recbox_amd__", False):
                assert getattr(mod, name) is getattr(matching, name), (path, name)
        layers = importlib.import_module("torch_rechub.basic.layers")
        if getattr(layers, "__recbox_amd__", False):
            assert layers.MultiInterestSA is ours.MultiInterestSA
    finally:
        compat.uninstall(report)


@pytest.mark.parametrize("shape", [(7, 16, 64, 4), (50, 64, 256, 4), (12, 32, 100, 3)])
def test_composition_matches_the_float64_restatement(shape):
    from recbox_amd import ops
    case = sa64.make_case(37, *shape)
    want = sa64.reference(case)
    got = sa64.run(ops.sa_pool_torch, case, "cpu")
    for name in ("out", "attn", "dx", "dw1", "dw2"):
        assert_close(got[name], want[name], 1e-4, name)
    got = sa64.run(ops.sa_pool, case, "cpu")                                    # the entry point the mirrors call
    for name in ("out", "attn", "dx", "dw1", "dw2"):
        assert_close(got[name], want[name], 1e-4, "sa_pool " + name)
    assert ops.sa_pool(case["x"], case["w1"], case["w2"], case["mask"], pool=False)[0] is None


def test_fully_masked_sample_in_the_restatement():
    case = sa64.make_case(5, 7, 16, 64, 4)
    want = sa64.reference(case)
    assert torch.equal(want["attn"][0], torch.full((7, 4), 1.0 / 7, dtype=torch.float64))
    assert float(want["dx"][0].abs().max()) > 0.0                               # the gradient passes the mask addition


@pytest.mark.parametrize("tag,cls", [("mind", "MIND"), ("comirec", "ComirecDR")])
def test_capsule_models_still_load_their_fixture_by_name(tag, cls):
    from recbox_amd.rechub.basic.features import SequenceFeature, SparseFeature
    from recbox_amd.rechub.models import matching
    fx = Fixture("rechub_multi_interest")
    user = [SparseFeature("user_id", vocab_size=11, embed_dim=D)]
    hist = [SequenceFeature("hist_item_id", vocab_size=23, embed_dim=D, pooling="concat", shared_with="item_id")]
    item = [SparseFeature("item_id", vocab_size=23, embed_dim=D)]
    neg = [SequenceFeature("neg_items", vocab_size=23, embed_dim=D, pooling="concat", shared_with="item_id")]
    model = getattr(matching, cls)(user, hist, item, neg, max_length=L, interest_num=K)
    assert set(model.state_dict().keys()) == set(fx["p_" + tag].keys())
    model.load_state_dict(fx.tensors("p_" + tag), strict=True)
    assert model.max_length == L and model.capsule.bilinear_type == (0 if tag == "mind" else 2)
    with pytest.raises(RuntimeError):                                           # still no CPU path for the capsule models
        model({k: v for k, v in fx.tensors("in").items()})
