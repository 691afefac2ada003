"""Expert-gate mixing on the GPU (``ops.expert_mix``: csrc/rbx_mix.hip) against the float64 restatement of tests/mix64.py, at
the smallest shapes where the kernels can go wrong, and MMOE / PLE / AITM against the live reference's fixture.

Forms the kernels dispatch: a sample is owned by a lane group of G = 1, 2, 4, 8, 16, 32, 64 lanes (H = 4, 8, 12 / 16, 32, 64,
128, 256; H = 12 leaves one lane of four idle), and from H = 260 on a lane owns 2, 3, 4 float4 columns (H = 260, 516, 1024).
A workgroup is four wavefronts: at H = 4 it owns 256 samples, so B = 300 fills more than one.

The fixture's MMOE and PLE mix experts of width 6, which is no multiple of 4: at the fixture's sizes they run the composition
(pinned to the reference here, switch on and off), and the fused path is shown on the same models with experts of width 8
against the composition.  AITM's width is 8: its fixture run goes through the kernels."""
import pytest
import torch

import mix64
from conftest import Fixture, assert_close

pytestmark = pytest.mark.gpu
TOL = 1e-4                                               # the project's contract (tests/test_gpu_din_unit.py, README)
FORMS = [4, 8, 12, 32, 64, 128, 256, 260, 516, 1024]
PLE = mix64.ple_select(2, 2, 1)                          # [[0, 1, 4], [2, 3, 4], [0 .. 4]]
ODD = [[2, 0], [0, 3, 2]]                                # expert 1 in no gate, 0 and 2 in every gate, not ascending


def _check(case, softmax=True, used=None, what=""):
    from recbox_amd import ops
    want = mix64.reference(case, softmax, used)
    got = mix64.run(ops.expert_mix, case, "cuda", softmax, used)
    for t, (a, b) in enumerate(zip(got["out"], want["out"])):
        assert_close(a, b, TOL, "%s out %d" % (what, t))
    for e, (a, b) in enumerate(zip(got["dx"], want["dx"])):
        assert_close(a, b, TOL, "%s dx %d" % (what, e))
    for t, (a, b) in enumerate(zip(got["dz"], want["dz"])):
        assert_close(a, b, TOL, "%s dz %d" % (what, t))
    return got


@pytest.fixture
def fused_only(monkeypatch):
    """For the duration of the test the composition raises: what passes went through the kernels."""
    from recbox_amd import ops

    def refuse(*a, **k):
        raise AssertionError("expert_mix_torch was called: the fused path did not run")
    assert ops.config.expert_mix_fused
    monkeypatch.setattr(ops, "expert_mix_torch", refuse)


@pytest.mark.parametrize("H", FORMS)
def test_every_form_against_float64(H, fused_only):
    _check(mix64.make_case(H, 37, H, 5, PLE), what="H=%d" % H)


@pytest.mark.parametrize("B", [1, 300])
@pytest.mark.parametrize("H", [4, 12, 260])
def test_batch_edges(B, H, fused_only):
    _check(mix64.make_case(B + H, B, H, 3, mix64.full_select(3, 2)), what="B=%d H=%d" % (B, H))


def test_one_expert_gives_weight_one_and_no_gate_gradient(fused_only):
    case = mix64.make_case(1, 37, 12, 1, [[0], [0]])
    got = _check(case, what="E=1")
    for t in range(2):
        assert torch.equal(got["out"][t].cpu(), case["x"][0])                  # p is exactly 1
        assert float(got["dz"][t].abs().max()) == 0.0


def test_widest_call(fused_only):
    _check(mix64.make_case(2, 37, 64, 16, mix64.full_select(16, 8)), what="E=16 T=8")


def test_single_gate(fused_only):
    _check(mix64.make_case(3, 37, 32, 3, mix64.full_select(3, 1)), what="T=1")


@pytest.mark.parametrize("softmax", [True, False])
def test_unused_shared_and_unordered_selection(softmax, fused_only):
    got = _check(mix64.make_case(4, 37, 16, 4, ODD), softmax, what="odd selection")
    assert float(got["dx"][1].abs().max()) == 0.0                               # selected by no gate: written, as zeros


def test_weights_without_softmax(fused_only):
    _check(mix64.make_case(5, 37, 128, 5, PLE), softmax=False, what="softmax=False")


def test_interleaved_rows_are_read_in_place(fused_only):
    """AITM's form: the two experts are rows 0 and 1 of one [B, 2, H] tensor (row stride 2 H)."""
    from recbox_amd import ops
    B, H = 37, 32
    case = mix64.make_case(6, B, H, 2, [[0, 1]])
    V = torch.stack(case["x"], dim=1).cuda().requires_grad_(True)
    assert ops._mix_rows(V[:, 1]).data_ptr() == V[:, 1].data_ptr() and V[:, 1].stride(0) == 2 * H
    want = mix64.reference(case)
    got = mix64.run(ops.expert_mix, case, "cuda", x_override=[V[:, 0], V[:, 1]], grad_z=False)
    assert_close(got["out"][0], want["out"][0], TOL, "interleaved out")
    got["loss"].backward()
    assert_close(V.grad, torch.stack(want["dx"], dim=1), TOL, "interleaved dV")


def test_extreme_logits_stay_finite_and_sum_to_one(fused_only):
    from recbox_amd import ops
    case = mix64.make_case(7, 37, 12, 4, mix64.full_select(4, 2))
    case["z"][0][3] = torch.tensor([80.0, -80.0, 79.0, -80.0])
    case["z"][1][5] = torch.tensor([-80.0, -80.0, -80.0, 80.0])
    got = _check(case, what="logits of +-80")
    assert all(bool(torch.isfinite(o).all()) for o in got["out"])
    ones = [torch.ones(37, 12, device="cuda") for _ in range(4)]
    for o in ops.expert_mix(ones, [z.cuda() for z in case["z"]]):
        assert_close(o, torch.ones(37, 12), TOL, "sum of the weights")


def test_an_output_without_gradient(fused_only):
    got = _check(mix64.make_case(8, 37, 16, 5, PLE), used={1}, what="loss over out_1 alone")
    assert float(got["dz"][0].abs().max()) == 0.0 and float(got["dz"][2].abs().max()) == 0.0
    assert float(got["dx"][0].abs().max()) == 0.0                               # expert 0 feeds gates 0 and 2 only


def test_gradients_for_one_side_only(fused_only):
    from recbox_amd import ops
    case = mix64.make_case(9, 37, 64, 5, PLE)
    want = mix64.reference(case)
    only_z = mix64.run(ops.expert_mix, case, "cuda", grad_x=False)
    only_x = mix64.run(ops.expert_mix, case, "cuda", grad_z=False)
    assert only_z["dx"] is None and only_x["dz"] is None
    for t, (a, b) in enumerate(zip(only_z["dz"], want["dz"])):
        assert_close(a, b, TOL, "gates only dz %d" % t)
    for e, (a, b) in enumerate(zip(only_x["dx"], want["dx"])):
        assert_close(a, b, TOL, "experts only dx %d" % e)


def test_two_runs_give_the_same_bits(fused_only):
    from recbox_amd import ops
    for H in (12, 128, 516):
        case = mix64.make_case(10, 300, H, 5, PLE)
        a, b = mix64.run(ops.expert_mix, case, "cuda"), mix64.run(ops.expert_mix, case, "cuda")
        for key in ("out", "dx", "dz"):
            for u, v in zip(a[key], b[key]):
                assert torch.equal(u, v), (H, key)


def test_outside_the_gate_the_composition_answers():
    from recbox_amd import ops
    for B, H, E, dtype in ((9, 6, 3, torch.float32), (9, 8, 17, torch.float32), (9, 8, 3, torch.float64), (0, 8, 3, torch.float32)):
        case = mix64.make_case(11, B, H, E, mix64.full_select(E, 2))
        x, z = [t.cuda().to(dtype) for t in case["x"]], [t.cuda().to(dtype) for t in case["z"]]
        got, want = ops.expert_mix(x, z), ops.expert_mix_torch(x, z)
        for a, b in zip(got, want):
            assert a.dtype == dtype and tuple(a.shape) == (B, H) and torch.equal(a, b)
    case = mix64.make_case(12, 9, 8, 3, mix64.full_select(3, 2))
    old = ops.config.expert_mix_fused
    try:
        ops.config.expert_mix_fused = False
        x, z = [t.cuda() for t in case["x"]], [t.cuda() for t in case["z"]]
        for a, b in zip(ops.expert_mix(x, z), ops.expert_mix_torch(x, z)):
            assert torch.equal(a, b)
    finally:
        ops.config.expert_mix_fused = old


# ---- models ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("tag", ["mmoe", "ple", "aitm"])
def test_models_match_the_reference_fixture(tag, fused, monkeypatch):
    from recbox_amd import ops
    monkeypatch.setattr(ops.config, "expert_mix_fused", fused)
    if fused and tag == "aitm":                          # width 8: the kernels serve it (MMOE / PLE at width 6: see the module docstring)
        monkeypatch.setattr(ops, "expert_mix_torch", lambda *a, **k: pytest.fail("the fused path did not run"))
    mix64.check_model_against_fixture(tag, "cuda", TOL)


def _wide(tag):
    """MMOE / PLE over the fixture's features with experts of width 8, which the kernels serve; seeded parameters."""
    import gen_golden_multi_task as gen
    from recbox_amd.rechub.basic import features
    from recbox_amd.rechub.models import multi_task
    sparse, seq, dense = gen.features(features)
    feats = sparse + [seq, dense]
    tower = {"dims": [4], "activation": "relu", "dropout": 0.0}
    expert = {"dims": [8, 8], "activation": "relu", "dropout": 0.0}
    if tag == "mmoe":
        model = multi_task.MMOE(feats, ["classification", "regression"], 3, expert, [dict(tower), dict(tower)])
    else:
        model = multi_task.PLE(feats, ["classification", "regression"], 2, 2, 1, expert, [dict(tower), dict(tower)])
    gen.seed_params(model, torch.Generator().manual_seed(41))
    return model.cuda().train()


def _step(model, x):
    y = model(x)
    y.sum().backward()
    return y


@pytest.mark.parametrize("tag", ["mmoe", "ple"])
def test_fused_models_equal_the_composition(tag, monkeypatch):
    from recbox_amd import ops
    x = Fixture("rechub_multi_task").tensors("in", "cuda")
    fused, plain = _wide(tag), _wide(tag)
    monkeypatch.setattr(ops.config, "expert_mix_fused", False)
    want = _step(plain, x)
    monkeypatch.setattr(ops.config, "expert_mix_fused", True)
    monkeypatch.setattr(ops, "expert_mix_torch", lambda *a, **k: pytest.fail("the fused path did not run"))
    got = _step(fused, x)
    assert_close(got, want, TOL, tag + " y")
    for (name, p), (_, q) in zip(fused.named_parameters(), plain.named_parameters()):
        assert (p.grad is None) == (q.grad is None), name
        if p.grad is not None:
            assert_close(p.grad, q.grad, TOL, "%s grad %s" % (tag, name))


# ---- capture -----------------------------------------------------------------------------------------------------------------
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


def test_capture_of_the_op_replays_the_eager_bits(fused_only):
    from recbox_amd import ops
    case = mix64.make_case(13, 300, 64, 5, PLE)
    eager = mix64.run(ops.expert_mix, case, "cuda")
    xs = [torch.zeros(300, 64, device="cuda").requires_grad_(True) for _ in range(5)]
    zs = [torch.zeros(300, len(s), device="cuda").requires_grad_(True) for s in PLE]
    ups = [u.cuda() for u in case["up"]]

    def step():
        outs = ops.expert_mix(xs, zs, PLE)
        sum((o * u).sum() for o, u in zip(outs, ups)).backward()
        return outs

    def zero():
        for t in xs + zs:
            t.grad = None
    graph, outs = _capture(step, zero)
    with torch.no_grad():
        for dst, src in zip(xs + zs, case["x"] + case["z"]):
            dst.copy_(src)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(list(outs) + [t.grad for t in xs] + [t.grad for t in zs], eager["out"] + eager["dx"] + eager["dz"]):
        assert torch.equal(a, b)


def test_capture_of_mmoe_replays_the_eager_bits(monkeypatch):
    """The fixture-sized MMOE with experts of width 8 (so that the kernels are in the graph), forward + backward in one graph."""
    from recbox_amd import ops
    monkeypatch.setattr(ops.config, "check_ids", False)                         # the id check reads the device
    monkeypatch.setattr(ops, "expert_mix_torch", lambda *a, **k: pytest.fail("the fused path did not run"))
    x = Fixture("rechub_multi_task").tensors("in", "cuda")
    eager, graphed = _wide("mmoe"), _wide("mmoe")
    want = _step(eager, x).detach()
    static = {k: torch.zeros_like(v) for k, v in x.items()}

    def zero():
        for p in graphed.parameters():
            p.grad = None
    graph, y = _capture(lambda: _step(graphed, static), zero)
    with torch.no_grad():
        for k, v in x.items():
            static[k].copy_(v)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y.detach(), want)
    for (name, p), (_, q) in zip(graphed.named_parameters(), eager.named_parameters()):
        assert (p.grad is None) == (q.grad is None), name
        if p.grad is not None:
            assert torch.equal(p.grad, q.grad), name
