"""The SENET gate and the bilinear pair op (``ops.senet_gate`` / ``ops.bilinear_pairs``, csrc/rbx_bilinear.hip) and the FiBiNet
mirror on the GPU: every output and gradient against the float64 restatement of tests/fibinet64.py under the fp32-scaled bar of
tests/fp32_bar.py (factor 4, its floor) over a paired shape grid; strided views; run-to-run bits; what the op refuses; one graph
capture of the model; the model against the live reference's fixture; peak memory against the composition."""
import ctypes

import pytest
import torch

import fibinet64
import fp32_bar
from conftest import Fixture

pytestmark = pytest.mark.gpu

# (B, F, D, transposed, with_scale, act): every B of {1, 15, 16, 17, 33, 257} (tile and chunk tails), every F of {2, 3, 5, 26}
# (P = 1, odd, the pair-group tail; R = 1 below F = 6), every D of {4, 8, 16, 32}, both layouts, scale present / absent, both
# gate activations -- paired, not multiplied, and run with each of the three kinds.
GRID = [(1, 2, 4, False, True, "relu"), (15, 3, 8, True, False, "sigmoid"), (16, 5, 16, False, True, "sigmoid"),
        (17, 26, 32, True, True, "relu"), (33, 5, 32, False, False, "relu"), (257, 26, 16, True, True, "relu"),
        (33, 3, 4, True, True, "sigmoid"), (17, 2, 8, False, True, "relu")]
_CACHE = {}


def _case(kind, B, F, D, tr, act, seed=11):
    key = (kind, B, F, D, tr, act, seed)
    if key not in _CACHE:
        case = fibinet64.make_case(seed, B, F, D, kind, act=act, transposed=tr)
        _CACHE[key] = (case, {ws: (fibinet64.reference(case, ws), fibinet64.reference(case, ws, torch.float32))
                              for ws in (True, False)})
    return _CACHE[key]


@pytest.fixture
def fused_only(monkeypatch):
    from recbox_amd import ops
    monkeypatch.setattr(ops.config, "bilinear_fused", True)
    monkeypatch.setattr(ops, "bilinear_pairs_torch", lambda *a, **k: pytest.fail("the fused pair op did not run"))
    monkeypatch.setattr(ops, "senet_gate_torch", lambda *a, **k: pytest.fail("the fused gate did not run"))


def _assert_all(tag, got, refs):
    want, ref32 = refs
    for name in fibinet64.NAMES:
        fp32_bar.assert_bar("%s %s" % (name, tag), got[name], want[name], ref32[name])


@pytest.mark.parametrize("kind", fibinet64.KINDS)
@pytest.mark.parametrize("shape", GRID, ids=lambda s: "B%d-F%d-D%d-%s-%s-%s" % (s[0], s[1], s[2], "oi" if s[3] else "io",
                                                                              "scale" if s[4] else "plain", s[5]))
def test_ops_match_float64_under_the_fp32_bar(kind, shape, fused_only):
    from recbox_amd import ops
    B, F, D, tr, ws, act = shape
    case, refs = _case(kind, B, F, D, tr, act)
    got = fibinet64.run(ops.senet_gate, ops.bilinear_pairs, case, "cuda", ws)
    _assert_all("%s %s" % (kind, shape), got, refs[ws])
    fp32_bar.report("fibinet %s %s" % (kind, (shape,)))


def test_grid_keeps_every_listed_value():
    assert {s[0] for s in GRID} == {1, 15, 16, 17, 33, 257} and {s[1] for s in GRID} == {2, 3, 5, 26}
    assert {s[2] for s in GRID} == {4, 8, 16, 32} and {s[3] for s in GRID} == {True, False}
    assert {s[4] for s in GRID} == {True, False} and {s[5] for s in GRID} == {"relu", "sigmoid"}


def test_x_is_read_as_a_view_of_a_wider_block(fused_only):
    from recbox_amd import ops
    case, refs = _case("field_each", 33, 5, 8, False, "relu")
    wide = torch.full((33, 5, 12), 7.0, device="cuda")
    wide[:, :, :8] = case["x"].cuda()
    wide.requires_grad_()
    got = fibinet64.run(ops.senet_gate, ops.bilinear_pairs, case, "cuda", True, x=(wide[:, :, :8], wide))
    assert float(got["dx"][:, :, 8:].abs().max()) == 0.0
    got["dx"] = got["dx"][:, :, :8]
    _assert_all("x view", got, refs[True])


def test_out_is_written_with_a_row_stride_and_nothing_else_is_touched():
    from recbox_amd import _lib
    case, refs = _case("field_interaction", 17, 5, 16, True, "relu")
    B, F, D, P = 17, 5, 16, 10
    x, W = case["x"].cuda(), case["W"].cuda()
    a = refs[True][0]["a"].float().cuda().contiguous()
    block = torch.full((B, 2 * P * D + 24), -3.0, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = _lib.lib.rbx_bilinear_pairs_fwd(x.data_ptr(), F * D, D, W.data_ptr(), a.data_ptr(), B, F, D, 2, 1, _lib.RBX_F32,
                                         block.data_ptr() + 8 * 4, block.stride(0), stream)
    assert rc == _lib.RBX_OK, _lib.last_error()
    torch.cuda.synchronize()
    assert bool((block[:, :8] == -3.0).all()) and bool((block[:, 8 + 2 * P * D:] == -3.0).all())
    want, ref32 = refs[True]
    fp32_bar.assert_bar("out strided", block[:, 8:8 + 2 * P * D].reshape(B, 2 * P, D), want["out"], ref32["out"])


def test_two_runs_give_the_same_bits(fused_only):
    from recbox_amd import ops
    case, _ = _case("field_interaction", 257, 26, 16, True, "relu")
    for kind in fibinet64.KINDS:
        c = case if kind == "field_interaction" else _case(kind, 257, 26, 16, True, "relu")[0]
        first = fibinet64.run(ops.senet_gate, ops.bilinear_pairs, c, "cuda", True)
        second = fibinet64.run(ops.senet_gate, ops.bilinear_pairs, c, "cuda", True)
        for name in fibinet64.NAMES:
            assert torch.equal(first[name], second[name]), (kind, name)


def test_refused_shapes_run_the_composition_and_still_match(monkeypatch):
    from recbox_amd import ops
    monkeypatch.setattr(_BilinearPairsGuard, "hits", 0)
    real = ops._BilinearPairs.apply
    monkeypatch.setattr(ops._BilinearPairs, "apply", lambda *a: _BilinearPairsGuard.hit(real, *a))
    case = fibinet64.make_case(5, 9, 4, 6, "field_each")                       # D = 6
    refs = (fibinet64.reference(case), fibinet64.reference(case, True, torch.float32))
    _assert_all("D=6", fibinet64.run(ops.senet_gate, ops.bilinear_pairs, case, "cuda", True), refs)
    case, refs = _case("field_all", 15, 3, 8, True, "sigmoid")
    wide = torch.zeros(15, 3, 16, device="cuda")
    wide[:, :, ::2] = case["x"].cuda()
    wide.requires_grad_()
    got = fibinet64.run(ops.senet_gate, ops.bilinear_pairs, case, "cuda", True, x=(wide[:, :, ::2], wide))
    got["dx"] = got["dx"][:, :, ::2]
    _assert_all("inner stride 2", got, refs[True])
    assert _BilinearPairsGuard.hits == 0


class _BilinearPairsGuard(object):
    hits = 0

    @classmethod
    def hit(cls, real, *a):
        cls.hits += 1
        return real(*a)


# ---- the model ---------------------------------------------------------------------------------------------------------------
def _step(model, x):
    y = model(x)
    y.sum().backward()
    return y


@pytest.mark.parametrize("kind", fibinet64.KINDS)
def test_model_matches_the_reference_and_both_routes_agree(kind, monkeypatch):
    from recbox_amd import ops
    monkeypatch.setattr(ops.config, "bilinear_fused", True)
    with monkeypatch.context() as m:
        m.setattr(ops, "bilinear_pairs_torch", lambda *a, **k: pytest.fail("the fused path did not run"))
        fused, y = fibinet64.check_model_against_fixture(kind, "cuda")
    monkeypatch.setattr(ops.config, "bilinear_fused", False)
    plain, y2 = fibinet64.check_model_against_fixture(kind, "cuda")
    # the lookup is the same kernel on the same ids whichever route the interaction takes
    x = Fixture("rechub_fibinet").tensors("in", "cuda")
    assert torch.equal(fused.embedding(x, fused.features), plain.embedding(x, plain.features))
    assert fibinet64.rel_err(y, y2) <= 1e-5


def test_capture_of_the_model_replays_the_eager_bits(monkeypatch):
    """Forward + backward of FiBiNet (B = 64, F = 5, D = 8) captured once on the default capture stream, replayed twice with new
    input contents."""
    import gen_golden_fibinet as gen
    from recbox_amd import ops
    monkeypatch.setattr(ops.config, "check_ids", False)                         # the id check reads the device
    monkeypatch.setattr(ops.config, "bilinear_fused", True)
    monkeypatch.setattr(ops, "bilinear_pairs_torch", lambda *a, **k: pytest.fail("the fused path did not run"))
    fx = Fixture("rechub_fibinet")
    eager, graphed = fibinet64.mirror("field_interaction"), fibinet64.mirror("field_interaction")
    for model in (eager, graphed):
        model.load_state_dict(fx.tensors("p_field_interaction"), strict=True)
        model.cuda().train()
    g = torch.Generator().manual_seed(3)
    batches = [{"s%d" % i: torch.randint(0, v, (64,), generator=g).cuda() for i, v in enumerate(gen.VOCABS)} for _ in range(2)]
    static = {k: torch.zeros_like(v) for k, v in batches[0].items()}

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            _step(graphed, static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for p in graphed.parameters():
        p.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = _step(graphed, static)
    for batch in batches:
        for p in eager.parameters():
            p.grad = None
        want = _step(eager, batch).detach()
        with torch.no_grad():
            for k, v in batch.items():
                static[k].copy_(v)
            for p in graphed.parameters():
                if p.grad is not None:
                    p.grad.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y.detach(), want)
        for (name, p), (_, q) in zip(graphed.named_parameters(), eager.named_parameters()):
            assert torch.equal(p.grad, q.grad), name


def test_peak_memory_is_below_the_composition():
    from recbox_amd import ops
    B, F, D = 2048, 26, 16
    g = torch.Generator().manual_seed(1)
    x0 = torch.randn(B, F, D, generator=g).cuda()
    W0 = (torch.randn(F * (F - 1) // 2, D, D, generator=g) * 0.3).cuda()
    a0 = torch.rand(B, F, generator=g).cuda()

    def peak(fn):
        x, W, a = x0.clone().requires_grad_(), W0.clone().requires_grad_(), a0.clone().requires_grad_()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn(x, W, "field_interaction", False, a)
        out.backward(out.detach())                     # the upstream gradient reuses no extra buffer beyond one of out's size
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    fused, plain = peak(ops.bilinear_pairs), peak(ops.bilinear_pairs_torch)
    print("peak bytes over forward + backward: fused %d, composition %d, ratio %.3f" % (fused, plain, fused / plain))
    assert fused < plain
