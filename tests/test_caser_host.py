"""Caser on the host: ``ops.caser_conv_torch`` (the reference's composition, which also serves what the fused op refuses) against
the float64 restatement of tests/caser64.py and against tests/golden/caser.npz (recorded from the live reference by
tests/gen_golden_caser.py); the mirrors ``recbole.CaserEncoder``, ``recbole.RegLoss`` and ``rechub.models.matching.Caser``
against the fixture's ``seq_output`` and every recorded gradient at 1e-4; the refusals.  No GPU."""
import pytest
import torch

import caser64 as cz
from conftest import Fixture, assert_close, assert_grads_close, load_params

CASES = ((37, 10, 16, 8, 4, 23), (19, 5, 8, 3, 0, 11), (11, 7, 4, 0, 2, 6))
N_USERS = 9
# (B, L, D, n_h, n_v): both parts, one height, no vertical part, no horizontal part, an odd filter count
SHAPES = [(5, 4, 8, 3, 2), (3, 1, 4, 1, 1), (4, 2, 8, 3, 0), (4, 7, 8, 0, 2), (6, 9, 12, 5, 3)]


def encoder(c):
    from recbox_amd import recbole
    B, L, D, n_h, n_v, n_items = CASES[c]
    return load_params(recbole.CaserEncoder(N_USERS, n_items, D, L, n_h, n_v), Fixture("caser")["p%d" % c])


def _composition(*a):
    from recbox_amd import ops
    return ops.caser_conv_torch(*a)


def _op(*a):
    from recbox_amd import ops
    return ops.caser_conv(*a)


@pytest.mark.parametrize("dims", SHAPES)
def test_composition_against_the_restatement(dims):
    case = cz.make_case(*dims)
    want = cz.reference(case)
    got = cz.run(_composition, case, "cpu", dtype=torch.float64)
    assert tuple(got["out"].shape) == (dims[0], dims[4] * dims[2] + dims[3] * dims[1])
    for n in ("out",) + cz.names(*dims[1:2], dims[3], dims[4]):
        assert_close(got[n], want[n], 1e-11, "%s %s" % (n, dims))


@pytest.mark.parametrize("dims", SHAPES)
def test_cpu_tensors_run_the_composition(dims):
    """Same bits as the composition, in float32 and in float64 (whose result stays float64)."""
    case = cz.make_case(*dims)
    for dtype in (torch.float32, torch.float64):
        a, b = cz.run(_op, case, "cpu", dtype=dtype), cz.run(_composition, case, "cpu", dtype=dtype)
        assert a["out"].dtype == dtype
        for n in a:
            assert torch.equal(a[n], b[n]), n


def test_composition_at_a_case_with_clear_winners():
    """What make_case promises, checked from outside: in float64 the best window of every (b, h, f) leads the runner-up by 1e-4
    of the largest pre-activation and is as far from zero.  With that the composition has the restatement's gradients."""
    case = cz.make_case(91, 10, 16, 8, 4)
    want, got = cz.reference(case), cz.run(_composition, case, "cpu", dtype=torch.float64)
    for n in want:
        assert_close(got[n], want[n], 1e-11, n)
    pre = cz.forward(case["x"].double(), None, None, [w.double() for w in case["w_h"]], [b.double() for b in case["b_h"]])[1]
    top = max(float(p.abs().max()) for p in pre)
    assert top == case["top"]
    for p in pre:
        best = p.topk(min(2, p.shape[1]), dim=1).values
        assert float(best[:, 0].abs().min()) >= cz.MARGIN * top
        if best.shape[1] == 2:
            assert float((best[:, 0] - best[:, 1]).min()) >= cz.MARGIN * top


def test_the_first_of_equal_windows_takes_the_gradient():
    """torch's max_pool1d rule, which the fused backward follows: a session of equal rows makes every window of a height equal."""
    from recbox_amd import ops
    L, D, n_h = 4, 4, 2
    x = torch.ones(1, L, D).requires_grad_()
    w_h = [torch.full((n_h, 1, h, D), 0.25) for h in range(1, L + 1)]
    b_h = [torch.zeros(n_h) for _ in range(L)]
    ops.caser_conv_torch(x, None, None, w_h, b_h).sum().backward()
    want = torch.tensor([sum(0.25 * n_h for h in range(1, L + 1) if h > l) for l in range(L)])
    assert torch.equal(x.grad[0, :, 0], want)


@pytest.mark.parametrize("c", [0, 1, 2])
def test_composition_against_the_reference_fixture(c):
    fx = Fixture("caser")
    B, L, D, n_h, n_v, n_items = CASES[c]
    m = encoder(c)
    emb = m.item_embedding(fx.tensors("in%d" % c)["seq"])
    assert_close(m.conv(emb), fx.tensors("out%d" % c)["conv"], 1e-5, "conv")


@pytest.mark.parametrize("c", [0, 1, 2])
def test_encoder_against_the_reference_fixture(c):
    fx = Fixture("caser")
    m = encoder(c).train()
    assert sorted(m.state_dict()) == sorted(fx["p%d" % c])
    x = fx.tensors("in%d" % c)
    y = m(x["user"], x["seq"])
    assert_close(y, fx.tensors("out%d" % c)["seq_output"], 1e-4, "seq_output")
    (y * x["up"]).sum().backward()
    assert_grads_close(m, fx.tensors("g%d" % c), 1e-4)


def test_state_dict_keys_and_initialisation():
    from recbox_amd import recbole
    torch.manual_seed(3)
    m = recbole.CaserEncoder(7, 13, 8, 5, 4, 2)
    keys = ["user_embedding.weight", "item_embedding.weight", "conv_v.weight", "conv_v.bias"]
    keys += ["conv_h.%d.%s" % (i, n) for i in range(5) for n in ("weight", "bias")] + ["fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias"]
    assert list(m.state_dict()) == keys
    assert tuple(m.conv_h[2].weight.shape) == (4, 1, 3, 8) and tuple(m.conv_v.weight.shape) == (2, 1, 5, 1)
    assert tuple(m.fc1.weight.shape) == (8, 2 * 8 + 4 * 5) and tuple(m.fc2.weight.shape) == (8, 16)
    assert float(m.fc1.bias.abs().max()) == 0.0 and float(m.fc2.bias.abs().max()) == 0.0
    assert float(m.item_embedding.weight.std()) < 0.3                      # normal_(0, 1 / D)


def test_reg_losses():
    from recbox_amd import recbole
    m = recbole.CaserEncoder(7, 13, 8, 5, 4, 2, reg_weight=0.5)
    want = 0.5 * sum(float(c.weight.norm(2)) for c in m.conv_h)
    assert abs(float(m.reg_loss_conv_h()) - want) <= 1e-6 * want
    ws = [m.user_embedding.weight, m.item_embedding.weight, m.conv_v.weight, m.fc1.weight, m.fc2.weight]
    assert abs(float(recbole.RegLoss()(ws)) - sum(float(w.norm(2)) for w in ws)) <= 1e-5
    assert recbole.RegLoss()([]) is None


def test_matching_model_scores_the_catalogue():
    from recbox_amd import compat
    from recbox_amd.rechub.basic.features import SequenceFeature, SparseFeature
    from recbox_amd.rechub.models.matching import Caser
    assert all("Caser" in names for path, names in compat.alias_also().items() if path.endswith(".models.matching"))
    c = 0
    B, L, D, n_h, n_v, n_items = CASES[c]
    fx = Fixture("caser")
    model = Caser(SparseFeature("user_id", N_USERS, D), SequenceFeature("hist_item_id", n_items, D, pooling="concat"), L, n_h, n_v,
                  dropout_prob=0.0)
    load_params(model.encoder, fx["p%d" % c])
    x = fx.tensors("in%d" % c)
    scores = model({"user_id": x["user"], "hist_item_id": x["seq"]})
    assert tuple(scores.shape) == (B, n_items)
    assert_close(scores, fx.tensors("out%d" % c)["seq_output"] @ model.encoder.item_embedding.weight.detach().t(), 1e-4, "scores")
    with pytest.raises(ValueError):
        Caser(SparseFeature("user_id", N_USERS, D), SequenceFeature("hist_item_id", n_items, D + 4, pooling="concat"), L)


def test_supported_class_and_refusals():
    from recbox_amd import ops
    ok = ops.caser_conv_supported
    assert ok(50, 64, 8, 4) and ok(10, 64, 8, 4) and ok(50, 64, 16, 8) and ok(1, 8, 1, 1) and ok(7, 8, 0, 2) and ok(2, 8, 3, 0)
    assert all(ok(L, D, 16, 8) for L in (1, 50) for D in (8, 16, 32, 64))
    assert not ok(51, 64, 8, 4) and not ok(0, 8, 1, 1)
    assert not ok(10, 6, 8, 4) and not ok(10, 68, 8, 4) and not ok(10, 0, 8, 4)
    assert not ok(10, 8, 17, 4) and not ok(10, 8, 8, 17) and not ok(10, 8, 0, 0)
    assert not ok(10, 8, 8, 4, torch.float64) and not ok(10, 8, 8, 4, torch.bfloat16)
    case = cz.make_case(3, 4, 8, 2, 1)
    x, w_v, b_v, w_h, b_h = case["x"], case["w_v"], case["b_v"], case["w_h"], case["b_h"]
    for bad in ((x[0], w_v, b_v, w_h, b_h), (x, w_v, None, w_h, b_h), (x, w_v, b_v, w_h[:3], b_h[:3]), (x, w_v, b_v, w_h, b_h[:3]),
                (x, w_v[:, :, :3], b_v, w_h, b_h), (x, w_v, b_v, w_h[::-1], b_h), (x, None, None, [], []),
                (x, w_v, b_v, w_h, [b.repeat(2) for b in b_h])):
        with pytest.raises(RuntimeError):
            ops.caser_conv(*bad)
    assert ops.caser_conv(x[:0], w_v, b_v, w_h, b_h).shape == (0, 1 * 8 + 2 * 4)
