"""FiGNN's fused message-passing step on the HIP path (csrc/rbx_fignn.hip: ops.fignn_step, recbole.FiGNNInteraction) against the
float64 restatement of tests/fignn64.py, every tensor under tests/fp32_bar.py's bar with factor 4 (``ref32`` the restatement in
fp32 on the CPU), and against tests/golden/fignn.npz (recorded from the live reference by tests/gen_golden_fignn.py).

A launch has min(256, ceil(tiles / 2)) workgroups that walk tiles of 16 samples, blockIdx first, then blockIdx + grid, ...:
B = 15 and 17 are one sample short of a tile and one past it; B = 91 is six tiles on three workgroups, so every workgroup takes
a second trip and the last one is partial (and adds into the dW_out / dW_in rows its first trip wrote); B = 549 leaves 18
per-workgroup rows and 72 per-wavefront rows, which the tail adds 16 rows at a time.  Where two [F][16][A + 4] buffers do not fit
in LDS (from 30 fields at A = 32) a tile is 8 samples: B = 37 at 39 x 32 is five tiles on three workgroups, B = 275 at 30 x 32
is 35 tiles on 18 workgroups."""
import functools

import pytest
import torch

import fignn64 as fg
import fp32_bar
from conftest import Fixture

pytestmark = pytest.mark.gpu
MAX_F_AT_32 = 48
# (F, A): the smallest; below a tile; A = 12; F a whole tile; one past it; the Criteo counts 26 and 39; A = 32; 39 x 32 and the
# largest F there, both on tiles of 8 samples
SHAPES = [(2, 4), (3, 8), (5, 12), (16, 16), (17, 16), (26, 16), (39, 16), (23, 32), (39, 32), (MAX_F_AT_32, 32)]


@pytest.fixture(autouse=True)
def _whole_range(monkeypatch):
    """Whatever the default gates are, these tests run the kernels over their whole range."""
    from recbox_amd import ops
    monkeypatch.setattr(ops.config, "fignn_fields", ops.FIGNN_MAX_FIELDS)
    monkeypatch.setattr(ops.config, "fignn_dim", ops.FIGNN_MAX_DIM)


@functools.lru_cache(maxsize=None)
def _case(B, F, A, same=False, seed=0, up_scale=1.0):
    """Above 60 000 leaky-relu arguments (B = 37 at 48 fields, B = 275 at 30) no seed keeps every one 1e-4 from zero at unit
    scale: w_attn is drawn 8 times wider there, which spreads the arguments and changes nothing else.  39 fields at B = 37
    stay at unit scale."""
    return fg.make_case(B, F, A, seed, same, 8.0 if B * F * F > 60000 else 1.0, up_scale)


@functools.lru_cache(maxsize=None)
def _refs(*key):
    case = _case(*key)
    return fg.reference(case), fg.ref32(case)


def _fused(*a):
    from recbox_amd import ops
    return ops.fignn_step(*a)


def _composition(*a):
    from recbox_amd import ops
    return ops.fignn_step_torch(*a)


def _check(got, refs, what, names=fg.NAMES):
    want, ref32 = refs
    for n in names:
        if want[n] is None:
            assert got[n] is None, n
        else:
            fp32_bar.assert_bar("%s %s" % (n, what), got[n], want[n], ref32[n])


def _same_bits(a, b, what="", names=fg.NAMES):
    for n in names:
        if a[n] is None or b[n] is None:
            assert a[n] is None and b[n] is None, n
        else:
            assert torch.equal(a[n], b[n]), "%s %s" % (what, n)


def _spy(monkeypatch):
    """Counts the calls that reach rbx_fignn_step_fwd."""
    from recbox_amd import ops
    calls = []
    fwd = ops.lib.rbx_fignn_step_fwd
    monkeypatch.setattr(ops.lib, "rbx_fignn_step_fwd", lambda *a: (calls.append(1), fwd(*a))[1])
    return calls


def test_largest_f_at_32():
    from recbox_amd import ops
    assert ops.fignn_step_supported(MAX_F_AT_32, 32) and not ops.fignn_step_supported(MAX_F_AT_32 + 1, 32)
    assert ops.lib.rbx_fignn_step_bwd_workspace_size(37, 39, 32) == 4 * 3 * (2 * 39 * 1024 + 2 * (6 * 1024 + 9 * 32))   # tiles of 8


@pytest.mark.parametrize("want_graph", [True, False])
@pytest.mark.parametrize("same", [False, True])
@pytest.mark.parametrize("B", [1, 37])
@pytest.mark.parametrize("F,A", SHAPES)
def test_every_shape_against_float64(monkeypatch, F, A, B, same, want_graph):
    from recbox_amd import ops
    assert ops.fignn_step_supported(F, A)
    calls = _spy(monkeypatch)
    key = (B, F, A, same)
    got = fg.run(_fused, _case(*key), "cuda", want_graph=want_graph)
    assert len(calls) == 1
    names = fg.NAMES if want_graph else tuple(n for n in fg.NAMES if n != "g")
    assert want_graph or got["g"] is None
    _check(got, _refs(*key), "F%d A%d B%d same%d" % (F, A, B, same), names)


# B = 549 only at 3 fields: at 17 fields its 149 328 leaky-relu arguments leave no seed with every one 1e-4 away from zero
# 30 x 32 runs on tiles of 8 samples: B = 275 is 35 tiles on 18 workgroups of 4 wavefronts, more rows than one chunk of the tail
@pytest.mark.parametrize("F,A,B,rows,nw", [(3, 8, 15, 1, 4), (3, 8, 17, 1, 4), (3, 8, 91, 3, 4), (3, 8, 549, 18, 4), (17, 16, 15, 1, 4),
                                           (17, 16, 17, 1, 4), (17, 16, 91, 3, 4), (23, 32, 91, 3, 2), (30, 32, 275, 18, 4)])
def test_batches_of_the_launch_geometry(F, A, B, rows, nw):
    from recbox_amd import ops
    assert ops.lib.rbx_fignn_step_bwd_workspace_size(B, F, A) == 4 * rows * (2 * F * A * A + nw * (6 * A * A + 9 * A))
    key = (B, F, A)
    _check(fg.run(_fused, _case(*key), "cuda"), _refs(*key), "F%d A%d B%d" % (F, A, B))


def test_gradient_subsets():
    """Only h (no workspace, no tail), only the weights, and each against the full run's bits."""
    from recbox_amd import ops
    case = _case(37, 5, 12)
    full = fg.run(_fused, case, "cuda")
    sizes = []
    size = ops.lib.rbx_fignn_step_bwd_workspace_size
    spy = lambda *a: (sizes.append(1), size(*a))[1]
    ops.lib.rbx_fignn_step_bwd_workspace_size = spy
    try:
        only_h = fg.run(_fused, case, "cuda", needs=(True,) + (False,) * 9)
        assert not sizes                                               # no weight gradient: no workspace is asked for
        only_w = fg.run(_fused, case, "cuda", needs=(False, False) + (True,) * 8)
        assert len(sizes) == 1
    finally:
        ops.lib.rbx_fignn_step_bwd_workspace_size = size
    assert torch.equal(only_h["dh"], full["dh"])
    assert all(only_h[n] is None for n in fg.GRADS[1:])
    assert only_w["dh"] is None and only_w["dh0"] is None
    _same_bits(only_w, full, "only the weights", fg.GRADS[2:])


def test_two_layer_chain_against_float64():
    """The second layer's h is the first one's output; h0 feeds both: every gradient of the chain."""
    case = _case(37, 7, 16, True)

    def chain(step):
        def fn(h, h0, *rest):
            ws, want_graph = rest[:8], rest[8]
            y, g = step(h, h0, *ws, want_graph)
            y2, _ = step(y, h0, *ws, False)
            return y2, g
        return fn
    got = fg.run(chain(_fused), case, "cuda")
    want = fg.run(chain(fg._literal), case, "cpu", dtype=torch.float64)
    ref32 = fg.run(chain(fg._literal), case, "cpu", dtype=torch.float32)
    _check(got, (want, ref32), "chain")


def test_two_runs_give_equal_bits():
    for key in ((549, 3, 8), (91, 17, 16)):
        case = _case(*key)
        _same_bits(fg.run(_fused, case, "cuda"), fg.run(_fused, case, "cuda"), "rerun %s" % (key,))


@pytest.mark.parametrize("F,A", [(7, 16), (26, 16)])                 # 26 x 16 takes more than 64 KiB of dynamic LDS
def test_graph_capture_replays_the_eager_bits(F, A):
    case = _case(37, F, A)
    eager = fg.run(_fused, case, "cuda")
    names = ("h", "h0") + fg.WEIGHTS
    t = [case[n].cuda().requires_grad_() for n in names]
    up = case["up"].cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                      # warm up off the default stream, as capture requires
        y, _ = _fused(*t, True)
        torch.autograd.grad((y * up).sum(), t)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y, g = _fused(*t, True)
        grads = torch.autograd.grad((y * up).sum(), t)
    for x in (y, g) + tuple(grads):
        x.detach().zero_()
    graph.replay()
    torch.cuda.synchronize()
    got = dict(zip(fg.GRADS, grads), y=y.detach(), g=g)
    _same_bits(got, eager, "replay")


def test_unsupported_classes_run_the_composition(monkeypatch):
    from recbox_amd import ops
    calls = _spy(monkeypatch)
    for F, A in ((5, 6), (49, 8), (5, 36)):
        assert not ops.fignn_step_supported(F, A)
        odd = fg.make_case(9, F, A)
        _same_bits(fg.run(_fused, odd, "cuda"), fg.run(_composition, odd, "cuda"), "refused F%d A%d" % (F, A))
    assert fg.run(_fused, _case(9, 5, 8), "cuda", dtype=torch.float64)["y"].dtype == torch.float64
    monkeypatch.setattr(ops.config, "fignn_fused", False)
    fg.run(_fused, _case(9, 5, 8), "cuda")
    assert not calls
    monkeypatch.setattr(ops.config, "fignn_fused", True)
    fg.run(_fused, _case(9, 5, 8), "cuda")
    assert len(calls) == 1


@pytest.mark.parametrize("c", [0, 1, 2])
def test_interaction_against_the_reference_fixture(monkeypatch, c):
    """The whole fignn_layer on the GPU, first stage on ops.field_attn; the project's fixture bar, 1e-4 on logits."""
    from recbox_amd import ops
    from test_fignn_host import CASES, interaction
    monkeypatch.setattr(ops.config, "field_attn_fields", ops.FIELD_ATTN_MAX_FIELDS)
    monkeypatch.setattr(ops.config, "field_attn_dim", ops.FIELD_ATTN_MAX_DIM)
    calls = _spy(monkeypatch)
    attn_calls = []
    fwd = ops.lib.rbx_fieldattn_fwd
    monkeypatch.setattr(ops.lib, "rbx_fieldattn_fwd", lambda *a: (attn_calls.append(1), fwd(*a))[1])
    fx = Fixture("fignn")
    m = interaction(c).cuda().train()
    x = fx.tensors("in%d" % c, "cuda")
    leaf = x["x"].clone().requires_grad_()
    y = m.fignn_layer(leaf)
    assert len(calls) == CASES[c][5] - 1 and len(attn_calls) == 1
    (y * x["up"]).sum().backward()
    out, g = fx.tensors("out%d" % c, "cuda"), fx.tensors("g%d" % c, "cuda")
    assert float((y.detach() - out["y"]).abs().max()) <= 1e-4
    assert float((m.graph - out["graph"]).abs().max()) <= 1e-5
    assert float((leaf.grad - g["x"]).abs().max()) <= 1e-4
    for name, p in m.named_parameters():
        if name in g:
            assert float((p.grad - g[name]).abs().max()) <= 1e-4, name


def test_report_worst_ratio():
    """Prints the worst err / bar per tensor over this module."""
    fp32_bar.report("fignn")
