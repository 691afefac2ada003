"""DCN-V2's cross expert mixture (``ops.cross_mix``, csrc/rbx_crossmix.hip) and the Deep & Cross mirrors on the GPU: every
output and gradient against the float64 restatement of tests/crossmix64.py under the fp32-scaled bar of tests/fp32_bar.py
(factor 4, its floor) over a paired shape grid; a strided x0; a strided out through the C ABI; run-to-run bits; what the op
refuses; the models against the live reference's fixture on both routes; one graph capture of DCNv2; peak memory against the
composition."""
import ctypes

import pytest
import torch

import crossmix64
import fp32_bar
from conftest import Fixture

pytestmark = pytest.mark.gpu

# (B, n, r, E, L): every B of {1, 15, 16, 17, 33, 257} (the row tile is 16; 257 rows are five chunks of the weight-gradient
# reduction, the last of one row), every n of {3, 16, 17, 40, 130, 416} (below one k-step of 4, on and beside the 16-column block,
# several blocks per wavefront, the workload's width), every r of {4, 8, 32, 64}, every E of {1, 2, 3, 4} and E r = 256 twice
# (4 x 64, 8 x 32), L of {1, 3} -- paired, not multiplied.
GRID = [(1, 3, 4, 1, 1), (15, 16, 8, 2, 3), (16, 17, 32, 3, 1), (17, 40, 64, 4, 3), (33, 130, 8, 4, 1), (257, 416, 32, 4, 3),
        (33, 40, 32, 8, 1), (17, 130, 4, 3, 3)]
_CACHE = {}


def _case(B, n, r, E, L, seed=11):
    key = (B, n, r, E, L, seed)
    if key not in _CACHE:
        case = crossmix64.make_case(seed, B, n, E, r, L)
        _CACHE[key] = (case, (crossmix64.reference(case), crossmix64.reference(case, torch.float32)))
    return _CACHE[key]


@pytest.fixture
def fused_only(monkeypatch):
    from recbox_amd import ops
    monkeypatch.setattr(ops.config, "crossmix_fused", True)
    monkeypatch.setattr(ops, "cross_mix_torch", lambda *a, **k: pytest.fail("the fused cross mixture did not run"))


def _assert_all(tag, got, refs, L):
    want, ref32 = refs
    for name in crossmix64.names(L):
        fp32_bar.assert_bar("%s %s" % (name, tag), got[name], want[name], ref32[name])


@pytest.mark.parametrize("shape", GRID, ids=lambda s: "B%d-n%d-r%d-E%d-L%d" % s)
def test_op_matches_float64_under_the_fp32_bar(shape, fused_only):
    from recbox_amd import ops
    B, n, r, E, L = shape
    case, refs = _case(B, n, r, E, L)
    got = crossmix64.run(ops.cross_mix, case, "cuda")
    _assert_all(str(shape), got, refs, L)
    fp32_bar.report("crossmix %s" % (shape,))


def test_grid_keeps_every_listed_value():
    assert {s[0] for s in GRID} == {1, 15, 16, 17, 33, 257} and {s[1] for s in GRID} == {3, 16, 17, 40, 130, 416}
    assert {s[2] for s in GRID} == {4, 8, 32, 64} and {s[3] for s in GRID} >= {1, 2, 3, 4} and {s[4] for s in GRID} == {1, 3}
    assert any(s[2] * s[3] == 256 for s in GRID)


def test_x0_is_read_as_a_view_of_a_wider_block(fused_only):
    from recbox_amd import ops
    case, refs = _case(33, 40, 32, 8, 1)
    wide = torch.full((33, 56), 7.0, device="cuda")
    wide[:, :40] = case["x0"].cuda()
    wide.requires_grad_()
    got = crossmix64.run(ops.cross_mix, case, "cuda", x0=(wide[:, :40], wide))
    assert float(got["dx0"][:, 40:].abs().max()) == 0.0
    got["dx0"] = got["dx0"][:, :40]
    _assert_all("x0 view", got, refs, 1)


def test_out_is_written_with_a_row_stride_and_nothing_else_is_touched():
    from recbox_amd import _lib
    case, refs = _case(33, 40, 32, 8, 1)
    B, n, E, r = 33, 40, 8, 32
    x0, G = case["x0"].cuda(), case["G"].cuda()
    U, V, C, b = (case[k][0].cuda().contiguous() for k in ("U", "V", "C", "b"))
    block = torch.full((B, n + 24), -3.0, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = _lib.lib.rbx_crossmix_fwd(x0.data_ptr(), n, x0.data_ptr(), n, U.data_ptr(), V.data_ptr(), C.data_ptr(), G.data_ptr(),
                                   b.data_ptr(), B, n, E, r, _lib.RBX_F32, block.data_ptr() + 8 * 4, block.stride(0), stream)
    assert rc == _lib.RBX_OK, _lib.last_error()
    torch.cuda.synchronize()
    assert bool((block[:, :8] == -3.0).all()) and bool((block[:, 8 + n:] == -3.0).all())
    want, ref32 = refs
    fp32_bar.assert_bar("out strided", block[:, 8:8 + n], want["out"], ref32["out"])


def test_two_runs_give_the_same_bits(fused_only):
    from recbox_amd import ops
    case, _ = _case(257, 416, 32, 4, 3)
    first, second = crossmix64.run(ops.cross_mix, case, "cuda"), crossmix64.run(ops.cross_mix, case, "cuda")
    for name in crossmix64.names(3):
        assert torch.equal(first[name], second[name]), name


class _NodeGuard(object):
    hits = 0

    @classmethod
    def hit(cls, real, *a):
        cls.hits += 1
        return real(*a)


def test_refused_shapes_run_the_composition_and_still_match(monkeypatch):
    from recbox_amd import ops
    monkeypatch.setattr(_NodeGuard, "hits", 0)
    real = ops._CrossMix.apply
    monkeypatch.setattr(ops._CrossMix, "apply", lambda *a: _NodeGuard.hit(real, *a))
    case = crossmix64.make_case(5, 9, 17, 2, 6, 2)                                # r = 6
    refs = (crossmix64.reference(case), crossmix64.reference(case, torch.float32))
    _assert_all("r=6", crossmix64.run(ops.cross_mix, case, "cuda"), refs, 2)
    case, refs = _case(15, 16, 8, 2, 3)
    wide = torch.zeros(15, 32, device="cuda")
    wide[:, ::2] = case["x0"].cuda()
    wide.requires_grad_()
    got = crossmix64.run(ops.cross_mix, case, "cuda", x0=(wide[:, ::2], wide))
    got["dx0"] = got["dx0"][:, ::2]
    _assert_all("inner stride 2", got, refs, 3)
    assert _NodeGuard.hits == 0


# ---- the models ---------------------------------------------------------------------------------------------------------------
def _step(model, x):
    y = model(x)
    y.sum().backward()
    return y


@pytest.mark.parametrize("which", crossmix64.MODELS)
def test_model_matches_the_reference_and_both_routes_agree(which, monkeypatch):
    from recbox_amd import ops
    monkeypatch.setattr(ops.config, "crossmix_fused", True)
    with monkeypatch.context() as m:
        m.setattr(ops, "cross_mix_torch", lambda *a, **k: pytest.fail("the fused path did not run"))
        _, y = crossmix64.check_model_against_fixture(which, "cuda")
    monkeypatch.setattr(ops.config, "crossmix_fused", False)
    _, y2 = crossmix64.check_model_against_fixture(which, "cuda")
    assert crossmix64.rel_err(y, y2) <= 1e-5


def test_capture_of_the_model_replays_the_eager_bits(monkeypatch):
    """Forward + backward of DCNv2 (parallel, mixture; B = 64, n = 40) captured once on the default capture stream, replayed
    twice with new input contents."""
    import gen_golden_crossmix as gen
    from recbox_amd import ops
    monkeypatch.setattr(ops.config, "check_ids", False)                         # the id check reads the device
    monkeypatch.setattr(ops.config, "crossmix_fused", True)
    monkeypatch.setattr(ops, "cross_mix_torch", lambda *a, **k: pytest.fail("the fused path did not run"))
    fx = Fixture("rechub_dcn")
    eager, graphed = crossmix64.mirror("v2par"), crossmix64.mirror("v2par")
    for model in (eager, graphed):
        model.load_state_dict(fx.tensors("p_v2par"), strict=True)
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
    for model in (eager, graphed):                                              # the warm-up moved the BatchNorm statistics
        model.load_state_dict(fx.tensors("p_v2par"), strict=True)
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
    B, n, E, r, L = 2048, 416, 4, 32, 3
    case = crossmix64.make_case(1, B, n, E, r, L)
    dev = {k: ([t.cuda() for t in v] if isinstance(v, list) else v.cuda()) for k, v in case.items() if k in ("x0", "G", "U", "V", "C", "b")}

    def peak(fn):
        leaf = lambda t: t.clone().requires_grad_()                               # noqa: E731
        x0, G = leaf(dev["x0"]), leaf(dev["G"])
        U, V, C, b = ([leaf(t) for t in dev[k]] for k in ("U", "V", "C", "b"))
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn(x0, U, V, C, G, b)
        out.backward(out.detach())
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    fused, plain = peak(ops.cross_mix), peak(ops.cross_mix_torch)
    print("peak bytes over forward + backward: fused %d, composition %d, ratio %.3f" % (fused, plain, fused / plain))
    assert fused < plain
