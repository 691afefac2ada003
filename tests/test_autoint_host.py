"""AutoInt without a GPU: the composition (ops.field_attn_torch), the mirrors (recbole.AutoIntInteraction, rechub's AutoInt)
against tests/golden/autoint.npz (recorded from the live reference by tests/gen_golden_autoint.py; the project's fixture bar,
1e-4 on logits) and against the float64 restatement of tests/fieldattn64.py; the composition against nn.MultiheadAttention bit
for bit; the dispatch rules of ops.field_attn; the C ABI's symbols and workspace size."""
import pytest
import torch

import fieldattn64 as fa
import fp32_bar
import test_gpu_autoint_forms as forms
from conftest import Fixture

TOL = 1e-4
CASES = ((37, 5, 8, 16, 2, 3, True), (19, 7, 16, 32, 4, 2, False))
MLP = [32, 16]


def interaction(c):
    """AutoIntInteraction of fixture case c with the recorded parameters (dropout 0)."""
    from recbox_amd.recbole import AutoIntInteraction
    B, F, D, A, h, layers, residual = CASES[c]
    m = AutoIntInteraction(F, D, A, layers, h, MLP, [0.0, 0.0, 0.0], residual)
    m.load_state_dict(Fixture("autoint").tensors("p%d" % c), strict=True)
    return m


def model_and_want(device="cpu"):
    """(model, ids, wanted scores): rechub-style AutoInt whose tables hold case 0's x (row b of table f = x[b, f]) and whose
    interaction holds its parameters, so the logit is the first-order term plus the recorded autoint_layer output."""
    from recbox_amd.rechub.basic.features import SparseFeature
    from recbox_amd.rechub.models.ranking import AutoInt
    fx = Fixture("autoint")
    B, F, D, A, h, layers, residual = CASES[0]
    x = fx.tensors("in0")["x"]
    torch.manual_seed(5)
    model = AutoInt([SparseFeature("s%d" % f, vocab_size=B, embed_dim=D) for f in range(F)], attention_size=A, n_layers=layers,
                    num_heads=h, mlp_hidden_size=MLP, dropout_probs=(0.0, 0.0, 0.0), has_residual=residual)
    model.interaction.load_state_dict(fx.tensors("p0"), strict=True)
    with torch.no_grad():
        for f in range(F):
            model.embedding.embed_dict["s%d" % f].weight.copy_(x[:, f])
    lin = model.linear.fc
    want = torch.sigmoid(x.flatten(1).double() @ lin.weight.detach().double().t() + lin.bias.detach().double()
                         + fx.tensors("out0")["y"].double()).squeeze(1)
    return model, {"s%d" % f: torch.arange(B, device=device) for f in range(F)}, want


def _close(a, b, what, tol=TOL):
    err = float((a.detach().double() - torch.as_tensor(b).double()).abs().max())
    assert err <= tol, "%s: %.3e" % (what, err)


@pytest.mark.parametrize("c", [0, 1])
def test_interaction_against_the_reference_fixture(c):
    fx = Fixture("autoint")
    m = interaction(c).train()
    x = fx.tensors("in%d" % c)
    leaf = x["x"].clone().requires_grad_()
    y = m(leaf)
    _close(y, fx["out%d" % c]["y"], "y")
    (y * x["up"]).sum().backward()
    _close(leaf.grad, fx["g%d" % c]["x"], "dx")
    for name, p in m.named_parameters():
        _close(p.grad, fx["g%d" % c][name], name)


@pytest.mark.parametrize("c", [0, 1])
def test_composition_layers_against_the_recorded_probabilities(c):
    """Layer by layer on the fixture's parameters: the per-head probabilities of every layer."""
    from recbox_amd import ops
    fx = Fixture("autoint")
    m = interaction(c)
    h = CASES[c][4]
    with torch.no_grad():
        cross = m.att_embedding(fx.tensors("in%d" % c)["x"])
        for i, attn in enumerate(m.self_attns):
            cross, p = ops.field_attn_torch(cross, attn.in_proj_weight, attn.in_proj_bias, attn.out_proj.weight,
                                            attn.out_proj.bias, h, want_attn=True)
            _close(p, fx["out%d" % c]["att%d" % i], "att%d" % i, 1e-6)


def test_state_dict_keys_are_the_references():
    for c in (0, 1):
        assert sorted(interaction(c).state_dict().keys()) == sorted(Fixture("autoint")["p%d" % c].keys())
    assert "v_res_embedding.weight" in interaction(0).state_dict() and "v_res_embedding.weight" not in interaction(1).state_dict()
    assert isinstance(interaction(0).self_attns[0], torch.nn.MultiheadAttention)


@pytest.mark.parametrize("res,relu,bias", [(False, False, True), (True, True, True), (True, False, False), (False, True, False)])
def test_composition_against_float64(res, relu, bias):
    case = fa.make_case(11, 7, 16, 2, res, relu, bias)
    want, got = fa.reference(case), fa.ref32(case)
    for n in fa.NAMES + ("attn",):
        if want[n] is None:
            assert got[n] is None, n
        else:
            assert tuple(got[n].shape) == tuple(want[n].shape), n
            scale = float(want[n].abs().max())
            _close(got[n], want[n], n, 2e-5 * max(scale, 1.0))


def test_the_form_cases_cover_every_form_of_the_launch_geometry():
    forms.check_the_list_covers_every_form()


def test_the_restatement_gives_the_wavefront_counts_the_form_list_was_chosen_from():
    """``forms`` restates fa_waves: three backward wavefronts exactly at FP 48 with E 12 and at FP 32 with E 24 or 28, and the
    shapes of tests/test_gpu_autoint.py reach backward counts of 4, 2 and 1 only; the three shapes closest to kFaLdsCap."""
    k = forms.constants()
    three = {(FP, E) for FP in (16, 32, 48) for E in range(4, 33, 4) if forms.forms(37, FP, E, k)["nw_bwd"] == 3}
    assert three == {(48, 12), (32, 24), (32, 28)}
    old = [(2, 4), (3, 8), (5, 12), (7, 16), (16, 16), (17, 16), (23, 32), (26, 16), (39, 16), (18, 32), (26, 32), (39, 32), (48, 32)]
    assert {forms.forms(37, F, E, k)["nw_bwd"] for F, E in old} == {4, 2, 1}
    for (FP, E), lds in forms.NEAR_CAP.items():
        assert forms.forms(37, FP, E, k)["bwd_lds"] == lds
    top = sorted((forms.forms(37, FP, E, k)["bwd_lds"] for FP in (16, 32, 48) for E in range(4, 33, 4)), reverse=True)
    assert top[:3] == sorted(forms.NEAR_CAP.values(), reverse=True) and top[0] <= k["kFaLdsCap"]
    assert forms.FORMS == [(False, False, True), (True, True, True), (True, False, False), (False, True, False)]


@pytest.mark.parametrize("name", list(forms.CASES))
def test_a_form_case_reaches_its_form_and_its_references_hold_the_bar(name):
    """What tests/test_gpu_autoint_forms.py sends to the GPU, judged here first: the case selects the launch geometry its table
    line names (the workspace rows read from the library), ``make_case`` finds a seed for it, the fp32 composition is finite and
    under the bar, and another fp32 order of the forward -- the restatement's own formulas in fp32 -- holds the same bar."""
    forms.check_forms(name)
    case = forms.make(name)
    want, ref32 = forms.refs(name)
    for n in forms.ALL:
        if want[n] is None:
            assert ref32[n] is None, n
            continue
        assert bool(torch.isfinite(ref32[n]).all()), n
        fp32_bar.assert_bar("%s ref32 %s" % (n, name), ref32[n], want[n], ref32[n])
    z, p = fa.forward64(case, dtype=torch.float32)[:2]
    fp32_bar.assert_bar("y restated-fp32 %s" % name, torch.relu(z) if case["relu"] else z, want["y"], ref32["y"])
    fp32_bar.assert_bar("attn restated-fp32 %s" % name, p, want["attn"], ref32["attn"])


@pytest.mark.parametrize("B,F,E,h", forms.DROP)
def test_the_dropout_form_cases_draw_a_seed(B, F, E, h):
    case = fa.make_case(B, F, E, h, True, True, True, 0.25)
    assert case["p"] == 0.25 and case["relu"] and forms.forms(B, F, E)["rows"] < B


def test_composition_under_a_keep_mask_against_float64():
    case = fa.make_case(11, 7, 16, 2, True, True, True, 0.25)
    keep = torch.rand(11 * 2, 7, 7, generator=torch.Generator().manual_seed(3)) >= 0.25
    want, got = fa.reference(case, keep), fa.ref32(case, keep)
    for n in fa.NAMES:
        _close(got[n], want[n], n, 2e-5 * max(float(want[n].abs().max()), 1.0))
    assert fa.drop_scale(0.25) == 4.0 / 3.0


@pytest.mark.parametrize("F,E,h", [(39, 16, 2), (5, 8, 1), (26, 32, 4)])
def test_composition_is_multihead_attention_bit_for_bit(F, E, h):
    from recbox_amd import ops
    torch.manual_seed(F)
    mha = torch.nn.MultiheadAttention(E, h)
    with torch.no_grad():
        mha.in_proj_bias.normal_()
        mha.out_proj.bias.normal_()
    x = torch.randn(11, F, E)
    fbe = x.transpose(0, 1).contiguous()
    with torch.no_grad():
        want, _ = mha(fbe, fbe, fbe)
        got, _ = ops.field_attn_torch(x, mha.in_proj_weight, mha.in_proj_bias, mha.out_proj.weight, mha.out_proj.bias, h)
    assert torch.equal(got, want.transpose(0, 1))


def test_cpu_tensors_run_the_composition_bit_for_bit():
    from recbox_amd import ops
    case = fa.make_case(11, 7, 16, 2, True, True)
    a = fa.run(ops.field_attn, case, "cpu")
    b = fa.run(ops.field_attn_torch, case, "cpu")
    for n in fa.NAMES + ("attn",):
        assert torch.equal(a[n], b[n]), n
    empty = ops.field_attn(torch.zeros(0, 7, 16), case["in_w"], case["in_b"], case["out_w"], case["out_b"], 2)[0]
    assert tuple(empty.shape) == (0, 7, 16)


def test_supported_table():
    from recbox_amd import ops
    for F in (2, 26, 39, 48):
        for E in range(4, 33, 4):
            for h in (1, 2, 3, 4, 8):
                want = E % h == 0 and (E // h) % 4 == 0
                assert ops.field_attn_supported(F, E, h) == want, (F, E, h)
    for F, E, h in ((1, 16, 2), (49, 16, 2), (39, 6, 1), (39, 36, 1), (39, 64, 2), (39, 16, 0), (39, 16, 16), (39, 8, 4)):
        assert not ops.field_attn_supported(F, E, h), (F, E, h)
    assert not ops.field_attn_supported(39, 16, 2, torch.float64)


def test_symbols_and_workspace_size():
    from recbox_amd import ops
    for name in ("rbx_fieldattn_supported", "rbx_fieldattn_fwd", "rbx_fieldattn_bwd_workspace_size", "rbx_fieldattn_bwd"):
        assert hasattr(ops.lib, name), name
    size = ops.lib.rbx_fieldattn_bwd_workspace_size
    row = 4 * (4 * 16 * 16 + 4 * 16)
    assert size(0, 39, 16, 2) == 0 and size(64, 40, 6, 1) == 0
    assert size(1, 39, 16, 2) % row == 0 and 0 < size(1, 39, 16, 2) <= 4 * row
    cap = size(1 << 20, 39, 16, 2)
    assert cap == size(1 << 24, 39, 16, 2) == size(1 << 16, 39, 16, 2)     # above the row cap the batch does not matter
    assert cap % row == 0 and cap // row <= 2048
    assert size(301, 39, 16, 2) < cap


def test_shape_errors_raise():
    from recbox_amd import ops
    x, wi, bi, wo, bo = torch.zeros(3, 5, 8), torch.zeros(24, 8), torch.zeros(24), torch.zeros(8, 8), torch.zeros(8)
    with pytest.raises(RuntimeError):
        ops.field_attn(x[0], wi, bi, wo, bo, 2)
    with pytest.raises(RuntimeError):
        ops.field_attn(x, wi[:16], bi, wo, bo, 2)
    with pytest.raises(RuntimeError):
        ops.field_attn(x, wi, bi[:8], wo, bo, 2)
    with pytest.raises(RuntimeError):
        ops.field_attn(x, wi, bi, wo[:, :4], bo, 2)
    with pytest.raises(RuntimeError):
        ops.field_attn(x, wi, bi, wo, bo, 3)
    with pytest.raises(RuntimeError):
        ops.field_attn(x, wi, bi, wo, bo, 2, residual=torch.zeros(3, 5, 4))
    with pytest.raises(ValueError):
        ops.field_attn(x, wi, bi, wo, bo, 2, dropout_p=1.0)
    with pytest.raises(RuntimeError):
        interaction(0)(torch.zeros(3, 6, 8))


def test_model_loads_the_fixture_and_trains():
    model, ids, want = model_and_want()
    model.eval()
    _close(model(ids), want, "scores")
    from recbox_amd import compat
    assert "AutoInt" in compat._RECHUB_ALSO["models.ranking"]
    model.train()
    torch.manual_seed(0)
    label = (torch.rand(CASES[0][0]) < 0.5).float()
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    losses = []
    for _ in range(8):
        opt.zero_grad()
        loss = torch.nn.functional.binary_cross_entropy(model(ids), label)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    assert losses[-1] < losses[0]


def test_training_dropout_applies_only_in_training():
    m = interaction(0)
    m.dropout_probs[0] = 0.5
    x = Fixture("autoint").tensors("in0")["x"]
    m.eval()
    _close(m(x), Fixture("autoint")["out0"]["y"], "eval ignores dropout")
    m.train()
    torch.manual_seed(1)
    assert float((m(x) - torch.from_numpy(Fixture("autoint")["out0"]["y"])).abs().max()) > 1e-3
