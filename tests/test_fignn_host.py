"""FiGNN without a GPU: the composition (ops.fignn_step_torch) against the float64 restatement of tests/fignn64.py under
tests/fp32_bar.py's bar (factor 4, ``ref32`` the restatement in fp32); the mirrors (recbole.FiGNNInteraction, rechub's FiGNN)
against tests/golden/fignn.npz, recorded from the live reference by tests/gen_golden_fignn.py.  The fixture comparisons use the
project's fixture rule, 1e-4 absolute on logits and gradients (the fixture itself is an fp32 run, so it cannot serve as the
``want`` of the float64 bar without a float64 recording); the graph, a softmax output, is held to 1e-6."""
import pytest
import torch

import fignn64 as fg
import fp32_bar
import test_gpu_fignn_forms as forms
from conftest import Fixture

TOL = 1e-4
CASES = ((37, 5, 8, 16, 2, 3), (19, 7, 16, 32, 4, 2), (11, 3, 4, 8, 1, 1))


def interaction(c):
    """FiGNNInteraction of fixture case c with the recorded parameters (dropouts 0)."""
    from recbox_amd.recbole import FiGNNInteraction
    B, F, D, A, h, layers = CASES[c]
    m = FiGNNInteraction(F, D, A, layers, h, 0.0, 0.0)
    m.load_state_dict(Fixture("fignn").tensors("p%d" % c), strict=True)
    return m


def _close(a, b, what, tol=TOL):
    err = float((a.detach().double() - torch.as_tensor(b).double()).abs().max())
    assert err <= tol, "%s: %.3e" % (what, err)


@pytest.mark.parametrize("B,F,A,same", [(11, 7, 16, False), (11, 7, 16, True), (5, 2, 4, False), (3, 39, 16, True), (4, 23, 32, False)])
def test_composition_against_float64(B, F, A, same):
    from recbox_amd import ops
    case = fg.make_case(B, F, A, 0, same)
    want, ref32 = fg.reference(case), fg.ref32(case)
    got = fg.run(ops.fignn_step_torch, case, "cpu")
    for n in fg.NAMES:
        if want[n] is None:
            assert got[n] is None, n
        else:
            fp32_bar.assert_bar("%s F%d A%d" % (n, F, A), got[n], want[n], ref32[n])


def test_the_form_cases_cover_every_form_of_the_launch_geometry():
    forms.check_the_list_covers_every_form()


def test_the_restatement_gives_the_ranges_the_kernel_file_quotes():
    """``forms`` restates fg_tile / fg_waves: it has to give the 16 -> 8 switches the .hip file's header quotes (46 x 20, 39 x 24,
    34 x 28, 30 x 32) and the ranges the form list was chosen from; the shapes of tests/test_gpu_fignn.py reach the forward with
    4 wavefronts only, and a lone backward wavefront never."""
    first8, combos = forms.header_figures()
    assert first8 == {20: 46, 24: 39, 28: 34, 32: 30}
    assert set(combos.values()) == forms.COMBOS

    def fields(A, pred):
        return [F for F in range(2, 49) if (F, A) in combos and pred(combos[(F, A)])]
    assert fields(16, lambda c: c[1] == 2) == [45, 46, 47, 48] and fields(20, lambda c: c[1] == 2) == [38, 39, 40, 41, 42, 43]
    assert fields(20, lambda c: c[1] == 1) == [44, 45] and fields(24, lambda c: c[1] == 1) == [38]
    lone = lambda c: c[0] == 16 and c[2] == 1
    assert fields(32, lone) == [26, 27, 28, 29] and fields(28, lone) == [30, 31, 32, 33] and fields(20, lone) == [42, 43, 44, 45]
    assert combos[(29, 32)] == (16, 4, 1)
    old = [(2, 4), (3, 8), (5, 12), (7, 16), (16, 16), (17, 16), (26, 16), (39, 16), (23, 32), (30, 32), (39, 32), (48, 32)]
    assert {combos[s] for s in old} == {(16, 4, 4), (16, 4, 2), (8, 4, 4), (8, 4, 2)}


@pytest.mark.parametrize("name", list(forms.CASES))
def test_a_form_case_reaches_its_form_and_its_references_hold_the_bar(name):
    """What tests/test_gpu_fignn_forms.py sends to the GPU, judged here first: the case selects the launch geometry its table
    line names (the workspace rows read from the library), ``make_case`` finds a seed for it, the fp32 restatement is finite and
    under the bar, and another fp32 summation order -- the composition on the CPU -- holds the same bar against float64."""
    from recbox_amd import ops
    forms.check_forms(name)
    case = forms.make(name)
    want, ref32 = forms.refs(name)
    got = fg.run(ops.fignn_step_torch, case, "cpu")
    for n in fg.NAMES:
        if want[n] is None:
            assert ref32[n] is None and got[n] is None, n
            continue
        assert bool(torch.isfinite(ref32[n]).all()), n
        fp32_bar.assert_bar("%s ref32 %s" % (n, name), ref32[n], want[n], ref32[n])
        fp32_bar.assert_bar("%s composition %s" % (n, name), got[n], want[n], ref32[n])


def test_cpu_tensors_and_empty_batches_run_the_composition():
    from recbox_amd import ops
    case = fg.make_case(11, 7, 16)
    a, b = fg.run(ops.fignn_step, case, "cpu"), fg.run(ops.fignn_step_torch, case, "cpu")
    for n in fg.NAMES:
        assert torch.equal(a[n], b[n]), n
    ws = [case[n] for n in fg.WEIGHTS]
    y, g = ops.fignn_step(torch.zeros(0, 7, 16), torch.zeros(0, 7, 16), *ws, want_graph=True)
    assert tuple(y.shape) == (0, 7, 16) and tuple(g.shape) == (0, 7, 7)
    with pytest.raises(RuntimeError):
        ops.fignn_step(case["h"], case["h0"][:, :5], *ws)
    with pytest.raises(RuntimeError):
        ops.fignn_step(case["h"], case["h0"], ws[0][:8], *ws[1:])


@pytest.mark.parametrize("c", [0, 1, 2])
def test_interaction_against_the_reference_fixture(c):
    fx = Fixture("fignn")
    m = interaction(c).train()
    assert sorted(m.state_dict().keys()) == sorted(fx["p%d" % c].keys())
    assert isinstance(m.self_attn, torch.nn.MultiheadAttention) and isinstance(m.gru_cell, torch.nn.GRUCell)
    x = fx.tensors("in%d" % c)
    leaf = x["x"].clone().requires_grad_()
    y = m.fignn_layer(leaf)
    assert tuple(y.shape) == (CASES[c][0], 1)
    _close(y, fx["out%d" % c]["y"], "y")
    _close(m.graph, fx["out%d" % c]["graph"], "graph", 1e-6)
    (y * x["up"]).sum().backward()
    _close(leaf.grad, fx["g%d" % c]["x"], "dx")
    recorded = fx["g%d" % c]
    for name, p in m.named_parameters():
        if name in recorded:
            _close(p.grad, recorded[name], name)
        else:                                                          # n_layers = 1: the reference gives these no gradient
            assert CASES[c][5] == 1 and (name == "W_attn.weight" or name.startswith("gru_cell.")), name
            assert p.grad is None, name


def test_one_layer_skips_the_steps(monkeypatch):
    from recbox_amd import ops
    calls = []
    monkeypatch.setattr(ops, "fignn_step", lambda *a, **k: calls.append(1))
    m = interaction(2)
    assert len(m.gnn) == 0
    m.fignn_layer(Fixture("fignn").tensors("in2")["x"])
    assert not calls


def test_compat_import_path():
    from recbox_amd import compat, recbole
    from recbox_amd.recbole.context_aware import FiGNNInteraction, GraphLayer
    from recbox_amd.rechub.models.ranking import FiGNN
    assert recbole.FiGNNInteraction is FiGNNInteraction and recbole.GraphLayer is GraphLayer
    assert all("FiGNN" in names for path, names in compat.alias_also().items() if path.endswith(".models.ranking"))
    import importlib
    report = compat.install()
    try:
        for root in ("torch_rechub", "recbox.third_party.rechub"):
            assert importlib.import_module(root + ".models.ranking").FiGNN is FiGNN, root
    finally:
        compat.uninstall(report)
    layer = GraphLayer(5, 8)
    assert tuple(layer.W_in.shape) == tuple(layer.W_out.shape) == (5, 8, 8) and float(layer.bias_p.detach().abs().max()) == 0.0
    assert tuple(layer(torch.softmax(torch.randn(3, 5, 5), -1), torch.randn(3, 5, 8)).shape) == (3, 5, 8)


def test_supported_at_its_limits():
    from recbox_amd import ops
    limits = {4: 48, 16: 48, 20: 48, 24: 48, 28: 48, 32: 48}
    for A, top in limits.items():
        assert ops.fignn_step_supported(2, A) and ops.fignn_step_supported(top, A), A
        assert not ops.fignn_step_supported(top + 1, A) and not ops.fignn_step_supported(1, A), A
    for F, A in ((5, 6), (5, 0), (5, 36), (0, 16)):
        assert not ops.fignn_step_supported(F, A), (F, A)
    assert not ops.fignn_step_supported(5, 8, torch.float64)
    size = ops.lib.rbx_fignn_step_bwd_workspace_size
    assert size(0, 39, 16) == 0 and size(64, 5, 6) == 0
    assert size(1 << 20, 39, 16) == size(1 << 24, 39, 16) == 4 * 256 * (2 * 39 * 256 + 4 * (6 * 256 + 9 * 16))


def test_model_runs_one_optimiser_step():
    from recbox_amd.rechub.basic.features import SparseFeature
    from recbox_amd.rechub.models.ranking import FiGNN
    torch.manual_seed(3)
    B, F, D = 12, 5, 8
    model = FiGNN([SparseFeature("s%d" % f, vocab_size=20, embed_dim=D) for f in range(F)], attention_size=16, n_layers=3,
                  num_heads=2, hidden_dropout=0.0, attn_dropout=0.0).train()
    ids = {"s%d" % f: torch.randint(0, 20, (B,)) for f in range(F)}
    label = (torch.rand(B) < 0.5).float()
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    before = [p.detach().clone() for p in model.parameters()]
    loss = torch.nn.functional.binary_cross_entropy(model(ids), label)
    loss.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
    opt.step()
    assert any(not torch.equal(a, p.detach()) for a, p in zip(before, model.parameters()))
