"""AFM without a GPU: the composition (ops.afm_pool_torch), the RecBole mirrors (recbole.layers.AttLayer,
recbole.context_aware.AFMInteraction) and rechub's AFM against tests/golden/afm.npz (recorded from the live reference by
tests/gen_golden_afm.py; fp32 CPU against fp32 CPU, 1e-5 absolute) and against the float64 restatement of tests/afm64.py; the
dispatch rules of ops.afm_pool; the C ABI's symbols."""
import pytest
import torch

import afm64
import fp32_bar
from conftest import Fixture

TOL = 1e-5
KEYS = ["p", "attlayer.h", "attlayer.w.weight"]


def _close(a, b, what, tol=TOL):
    err = float((a.detach().double() - torch.as_tensor(b).double()).abs().max())
    assert err <= tol, "%s: %.3e" % (what, err)


def _interaction(c):
    from recbox_amd.recbole.context_aware import AFMInteraction
    fx = Fixture("afm")
    B, F, D = fx["in%d" % c]["x"].shape
    m = AFMInteraction(F, D, fx["p%d" % c]["attlayer.h"].shape[0], 0.0)
    m.load_state_dict(fx.tensors("p%d" % c), strict=True)
    return fx, m


@pytest.mark.parametrize("c", [0, 1])
def test_composition_against_the_reference_fixture(c):
    from recbox_amd import ops
    fx = Fixture("afm")
    t, p = fx.tensors("in%d" % c), fx.tensors("p%d" % c)
    out, attn = ops.afm_pool_torch(t["x"], p["attlayer.w.weight"], p["attlayer.h"], want_attn=True)
    _close(attn, fx["out%d" % c]["att"], "attn")
    _close((out * p["p"]).sum(1, keepdim=True), fx["out%d" % c]["y"], "y")
    assert ops.afm_pool_torch(t["x"], p["attlayer.w.weight"], p["attlayer.h"])[1] is None


@pytest.mark.parametrize("c", [0, 1])
def test_mirrors_against_the_reference_fixture(c):
    fx, m = _interaction(c)
    t = fx.tensors("in%d" % c)
    assert list(m.state_dict().keys()) == KEYS and list(m.attlayer.state_dict().keys()) == ["h", "w.weight"]
    _close(m.attlayer(t["z"]), fx["out%d" % c]["att_z"], "AttLayer")
    x = t["x"].clone().requires_grad_()
    y = m(x)
    assert tuple(y.shape) == (x.shape[0], 1)
    (y * t["up"]).sum().backward()
    _close(y, fx["out%d" % c]["y"], "y")
    _close(m.attention(x), fx["out%d" % c]["att"], "att")
    _close(x.grad, fx["g%d" % c]["x"], "dx")
    for name, p in m.named_parameters():
        _close(p.grad, fx["g%d" % c][name], "grad " + name)
    _close(m.reg_loss(0.5), 0.5 * float(torch.linalg.norm(m.attlayer.w.weight.detach().double())), "reg_loss")


def test_init_weights_and_constructor():
    from recbox_amd.recbole.context_aware import AFMInteraction
    from recbox_amd.recbole.layers import AttLayer
    layer = AttLayer(8, 25)
    assert (layer.in_dim, layer.att_dim) == (8, 25) and layer.w.bias is None and tuple(layer.h.shape) == (25,)
    torch.manual_seed(0)
    m = AFMInteraction(6, 64, 64, 0.3)
    assert isinstance(m.dropout_layer, torch.nn.Dropout) and m.dropout_layer.p == 0.3 and m.num_pair == 15
    assert abs(float(m.attlayer.w.weight.detach().std()) -(2.0 / 128) ** 0.5) < 0.01          # xavier normal
    with pytest.raises(RuntimeError, match="5, 64"):
        m(torch.zeros(2, 5, 64))


@pytest.mark.parametrize("dims", [(3, 2, 4, 1), (5, 5, 8, 25), (4, 7, 16, 32), (3, 6, 20, 7)])
def test_composition_against_float64(dims):
    from recbox_amd import ops
    case = afm64.make_case(*dims)
    want, ref32 = afm64.reference(case), afm64.reference(case, dtype=torch.float32)
    got = afm64.run(ops.afm_pool_torch, case, "cpu")
    for n in afm64.NAMES:
        fp32_bar.assert_bar("%s %s" % (n, dims), got[n], want[n], ref32[n])
    if dims[1] > 2:
        assert case["zeros"] > 0


def test_cpu_tensors_run_the_composition_bit_for_bit():
    from recbox_amd import ops
    case = afm64.make_case(9, 7, 16, 32)
    a, b = afm64.run(ops.afm_pool, case, "cpu"), afm64.run(ops.afm_pool_torch, case, "cpu")
    for n in afm64.NAMES:
        assert torch.equal(a[n], b[n]), n
    out, attn = ops.afm_pool(torch.zeros(0, 5, 8), torch.zeros(3, 8), torch.zeros(3), want_attn=True)      # an empty batch
    assert tuple(out.shape) == (0, 8) and tuple(attn.shape) == (0, 10)
    out, _ = ops.afm_pool(case["x"].double(), case["w"].double(), case["h"].double())                       # not float32
    assert out.dtype == torch.float64


def test_supported_table():
    from recbox_amd import ops
    ok = ops.afm_pool_supported
    for F in (2, 26, 39):
        for D in range(4, 65, 4):
            for A in (1, 25, 33, 64):
                assert ok(F, D, A), (F, D, A)
    for F, D, A in ((1, 16, 25), (40, 16, 25), (5, 6, 25), (5, 2, 25), (5, 68, 25), (5, 0, 25), (5, 16, 0), (5, 16, 65)):
        assert not ok(F, D, A), (F, D, A)
    assert not ok(5, 16, 25, torch.bfloat16) and not ok(5, 16, 25, torch.float64)
    assert (ops.AFM_MAX_FIELDS, ops.AFM_MAX_DIM, ops.AFM_MAX_ATT) == (39, 64, 64)


def test_symbols_and_workspace_size():
    from recbox_amd import ops
    for name in ("rbx_afm_supported", "rbx_afm_fwd", "rbx_afm_bwd_workspace_size", "rbx_afm_bwd"):
        assert hasattr(ops.lib, name), name
    size = ops.lib.rbx_afm_bwd_workspace_size
    assert size(0, 5, 8, 25) == 0 and size(37, 40, 8, 25) == 0
    assert size(1, 5, 8, 25) == 4 * 4 * (25 * 8 + 25)                  # one workgroup of four wavefronts
    assert size(10 ** 6, 5, 8, 25) == 2048 * 4 * (25 * 8 + 25)         # capped at 512 workgroups
    assert size(10 ** 6, 39, 64, 64) == 512 * 4 * (64 * 64 + 64)       # one wavefront per workgroup where LDS allows no more


def test_shape_errors_raise():
    from recbox_amd import ops
    x, w, h = torch.zeros(3, 5, 8), torch.zeros(4, 8), torch.zeros(4)
    for bad in ((x[0], w, h), (x, w[:, :4], h), (x, w, h[:3]), (x, w[0], h)):
        with pytest.raises(RuntimeError, match=r"afm_pool: x \("):
            ops.afm_pool(*bad)


def test_model_constructs_trains_and_loads_the_fixture():
    from recbox_amd import compat
    from recbox_amd.rechub.basic.features import SparseFeature
    from recbox_amd.rechub.models import ranking
    fx = Fixture("afm")
    torch.manual_seed(3)
    feats = [SparseFeature("s%d" % f, vocab_size=11 + f, embed_dim=8) for f in range(5)]
    model = ranking.AFM(feats, attention_size=25, dropout_prob=0.3)
    assert [k for k in model.state_dict() if k.startswith("interaction.")] == ["interaction." + k for k in KEYS]
    model.interaction.load_state_dict(fx.tensors("p0"), strict=True)
    g = torch.Generator().manual_seed(4)
    with torch.no_grad():                                              # rechub's default tables are N(0, 1e-4): pair products of 1e-8
        for table in model.embedding.embed_dict.values():
            table.weight.copy_(torch.randn(table.weight.shape, generator=g) * 0.5)
    x = {"s%d" % f: torch.randint(0, 11 + f, (16,), generator=g) for f in range(5)}
    label = torch.randint(0, 2, (16,), generator=g).float()
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    model.train()
    y = model(x)
    assert tuple(y.shape) == (16,) and bool(((y > 0) & (y < 1)).all())
    loss = torch.nn.functional.binary_cross_entropy(y, label) + model.interaction.reg_loss(1e-3)
    loss.backward()
    before = [p.detach().clone() for p in model.parameters()]
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
    opt.step()
    for a, (name, b) in zip(before, model.named_parameters()):
        assert not torch.equal(a, b), name
    with pytest.raises(ValueError):
        ranking.AFM(feats[:1])
    assert all("AFM" in names for path, names in compat.alias_also().items() if path.endswith(".models.ranking"))
    assert not any(path.startswith("recbole") or ".recbole" in path for path in compat.alias_table())
