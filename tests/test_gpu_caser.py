"""Caser's fused convolutions on the HIP path (csrc/rbx_caser.hip: ops.caser_conv, recbole.CaserEncoder) against the float64
restatement of tests/caser64.py, every tensor under tests/fp32_bar.py's bar with factor 4 (``ref32`` the restatement in fp32 on
the CPU), and against tests/golden/caser.npz (recorded from the live reference by tests/gen_golden_caser.py).

The launch constants of rbx_caser.hip that the batches below are derived from.  The forward has min(tiles, 256) workgroups (one per
compute unit) that walk tiles of 16 samples, blockIdx first, then blockIdx + grid, ...: B = 15 and 17 are one sample short of a
tile and one past it; B = 8190 is 512 tiles on 256 workgroups, so every workgroup takes a second trip and the last tile holds 14
samples.  The dx kernel has min(4096, ceil(B / 2)) workgroups of one sample each: at B = 94 all 47 take a second one, at
B = 8190 all 4095.  The weight gradients are one thread per element (P = n_h D L (L + 1) / 2 + n_h L + n_v L + n_v = 28 284 at
10 x 64 x 8 x 4, 111 chunks of 256) and R = min(32, ceil(4096 / chunks), ceil(B / 32)) runs of ceil(B / R) samples: B = 94 is
three runs of 32, 32 and 30; B = 549 is 18 runs (17 of 31 samples and one of 22), more workspace rows than the 16 the tail adds
at once; B = 8190 is 32 runs, 31 of 256 samples and one of 254.  Where 16 rows of L D + 4 floats and the staged w_v do not fit in
160 KiB of LDS (L D + pad4(L) > 2552: both 50 x 64 shapes) a tile is 8 samples: B = 9 there is two tiles, the second of one
sample, on two workgroups."""
import functools

import pytest
import torch

import caser64 as cz
import fp32_bar
from conftest import Fixture

pytestmark = pytest.mark.gpu
# (L, D, n_h, n_v): one height and one window; no vertical part; no horizontal part; a small one; the advised setting; a whole
# MFMA tile of window rows and one past it; n_h no multiple of 4; the default at full length and the largest, on tiles of 8
SHAPES = [(1, 8, 1, 1), (2, 8, 3, 0), (7, 8, 0, 2), (5, 16, 8, 4), (10, 64, 8, 4), (16, 16, 16, 8), (17, 16, 16, 8), (23, 32, 5, 3),
          (50, 64, 8, 4), (50, 64, 16, 8)]
ADVISED = (10, 64, 8, 4)


@pytest.fixture(autouse=True)
def _whole_range(monkeypatch):
    """Whatever the default routing is, these tests run the kernels over their whole range."""
    from recbox_amd import ops
    monkeypatch.setattr(ops.config, "caser_fused", True)
    monkeypatch.setattr(ops, "CASER_FUSED_MAX_LEN", ops.CASER_MAX_LEN)
    monkeypatch.setattr(ops, "CASER_FUSED_MAX_BATCH", 1 << 40)
    monkeypatch.setattr(ops, "CASER_FUSED_LONG_MAX_BATCH", 1 << 40)


def _batch(L, D):
    return 9 if L * D + (L + 3) // 4 * 4 > 2552 else 37


@functools.lru_cache(maxsize=None)
def _case(B, L, D, n_h, n_v):
    return cz.make_case(B, L, D, n_h, n_v)


@functools.lru_cache(maxsize=None)
def _refs(*key):
    case = _case(*key)
    return cz.reference(case), cz.ref32(case)


def _fused(*a):
    from recbox_amd import ops
    return ops.caser_conv(*a)


def _check(got, refs, what):
    want, ref32 = refs
    assert sorted(got) == sorted(want)
    for n in want:
        fp32_bar.assert_bar("%s %s" % (n, what), got[n], want[n], ref32[n])


def _same_bits(a, b, what=""):
    assert sorted(a) == sorted(b)
    for n in a:
        assert torch.equal(a[n], b[n]), "%s %s" % (what, n)


def _spy(monkeypatch):
    """Counts the calls that reach rbx_caser_fwd."""
    from recbox_amd import ops
    calls = []
    fwd = ops.lib.rbx_caser_fwd
    monkeypatch.setattr(ops.lib, "rbx_caser_fwd", lambda *a: (calls.append(1), fwd(*a))[1])
    return calls


def _elements(L, D, n_h, n_v):
    return n_h * D * L * (L + 1) // 2 + n_h * L + n_v * L + n_v


@pytest.mark.parametrize("L,D,n_h,n_v", SHAPES)
def test_every_shape_against_float64(monkeypatch, L, D, n_h, n_v):
    from recbox_amd import ops
    assert ops.caser_conv_supported(L, D, n_h, n_v)
    calls = _spy(monkeypatch)
    key = (_batch(L, D), L, D, n_h, n_v)
    got = cz.run(_fused, _case(*key), "cuda")
    assert len(calls) == 1
    _check(got, _refs(*key), "L%d D%d nh%d nv%d B%d" % (L, D, n_h, n_v, key[0]))


@pytest.mark.parametrize("B,runs", [(1, 1), (15, 1), (17, 1), (94, 3), (549, 18), (8190, 32)])
def test_batches_of_the_launch_geometry(B, runs):
    from recbox_amd import ops
    assert ops.lib.rbx_caser_bwd_workspace_size(B, *ADVISED) == 4 * runs * _elements(*ADVISED)
    key = (B,) + ADVISED
    _check(cz.run(_fused, _case(*key), "cuda"), _refs(*key), "B%d" % B)


def test_reduced_tile_workspace():
    from recbox_amd import ops
    assert ops.lib.rbx_caser_bwd_workspace_size(9, 50, 64, 16, 8) == 4 * 1 * _elements(50, 64, 16, 8)
    assert ops.lib.rbx_caser_bwd_workspace_size(0, 50, 64, 16, 8) == 0 and ops.lib.rbx_caser_bwd_workspace_size(9, 51, 64, 16, 8) == 0


@pytest.mark.parametrize("L,D,n_h,n_v", [(5, 16, 8, 4), ADVISED])
def test_strided_x_is_read_in_place(monkeypatch, L, D, n_h, n_v):
    """x is the leading D columns of rows of D + 8 floats."""
    calls = _spy(monkeypatch)
    key = (37, L, D, n_h, n_v)

    def wide(x, dtype):
        leaf = torch.randn(x.shape[0], L, D + 8, device=x.device)
        leaf[:, :, :D] = x
        leaf.requires_grad_()
        return leaf, leaf[:, :, :D]
    got = cz.run(_fused, _case(*key), "cuda", x_view=wide)
    assert len(calls) == 1
    _check(got, _refs(*key), "strided L%d D%d" % (L, D))


def test_gradient_subsets():
    """Only x (no workspace, no tail), only the parameters, and each against the full run's bits."""
    from recbox_amd import ops
    case = _case(37, 5, 16, 8, 4)
    full = cz.run(_fused, case, "cuda")
    t = [case["x"].cuda().requires_grad_(), case["w_v"].cuda(), case["b_v"].cuda(), [w.cuda() for w in case["w_h"]],
         [b.cuda() for b in case["b_h"]]]
    up = case["up"].cuda()
    sizes = []
    size = ops.lib.rbx_caser_bwd_workspace_size
    ops.lib.rbx_caser_bwd_workspace_size = lambda *a: (sizes.append(1), size(*a))[1]
    try:
        (dx,) = torch.autograd.grad((_fused(*t) * up).sum(), [t[0]])
        assert not sizes                                               # no weight gradient: no workspace is asked for
        t[0] = t[0].detach()
        t[3] = [w.requires_grad_() for w in t[3]]
        dws = torch.autograd.grad((_fused(*t) * up).sum(), t[3])
        assert len(sizes) == 1
    finally:
        ops.lib.rbx_caser_bwd_workspace_size = size
    assert torch.equal(dx, full["dx"])
    for i, dw in enumerate(dws):
        assert torch.equal(dw, full["dw_h%d" % i]), i


def test_two_runs_give_equal_bits():
    for key in ((549,) + ADVISED, (37, 23, 32, 5, 3), (9, 50, 64, 8, 4)):
        case = _case(*key)
        _same_bits(cz.run(_fused, case, "cuda"), cz.run(_fused, case, "cuda"), "rerun %s" % (key,))


@pytest.mark.parametrize("L,D,n_h,n_v", [ADVISED, (20, 64, 16, 4)])           # 20 x 64 takes more than 64 KiB of dynamic LDS
def test_graph_capture_replays_the_eager_bits(L, D, n_h, n_v):
    case = _case(37, L, D, n_h, n_v)
    eager = cz.run(_fused, case, "cuda")
    x = case["x"].cuda().requires_grad_()
    w_v, b_v = case["w_v"].cuda().requires_grad_(), case["b_v"].cuda().requires_grad_()
    w_h = [w.cuda().requires_grad_() for w in case["w_h"]]
    b_h = [b.cuda().requires_grad_() for b in case["b_h"]]
    t = [x, w_v, b_v] + w_h + b_h
    up = case["up"].cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                      # warm up off the default stream, as capture requires
        y = _fused(x, w_v, b_v, w_h, b_h)
        torch.autograd.grad((y * up).sum(), t)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = _fused(x, w_v, b_v, w_h, b_h)
        grads = torch.autograd.grad((y * up).sum(), t)
    for g in (y,) + tuple(grads):
        g.detach().zero_()
    graph.replay()
    torch.cuda.synchronize()
    got = dict(zip(cz.names(L, n_h, n_v), grads), out=y.detach())
    _same_bits(got, eager, "replay")


def test_unsupported_classes_run_the_composition(monkeypatch):
    from recbox_amd import ops
    calls = _spy(monkeypatch)
    for dims in ((9, 4, 6, 2, 1), (5, 3, 68, 2, 1), (5, 3, 8, 17, 1), (5, 3, 8, 2, 17)):
        assert not ops.caser_conv_supported(*dims[1:])
        odd = cz.make_case(*dims)
        # (not compared with a second run of the composition bit for bit: its convolution backward does not repeat its bits)
        _check(cz.run(_fused, odd, "cuda"), (cz.reference(odd), cz.ref32(odd)), "refused %s" % (dims,))
        assert not calls
    small = _case(9, 4, 8, 2, 1)
    assert cz.run(_fused, small, "cuda", dtype=torch.float64)["out"].dtype == torch.float64
    monkeypatch.setattr(ops, "CASER_FUSED_MAX_LEN", 3)
    cz.run(_fused, small, "cuda")
    monkeypatch.setattr(ops, "CASER_FUSED_MAX_LEN", ops.CASER_MAX_LEN)
    monkeypatch.setattr(ops, "CASER_FUSED_MAX_BATCH", 8)
    cz.run(_fused, small, "cuda")
    monkeypatch.setattr(ops, "CASER_FUSED_MAX_BATCH", 1 << 40)
    monkeypatch.setattr(ops, "CASER_FUSED_LONG_LEN", 3)                # a long session in a batch above the long sessions' bound
    monkeypatch.setattr(ops, "CASER_FUSED_LONG_MAX_BATCH", 8)
    cz.run(_fused, small, "cuda")
    monkeypatch.setattr(ops, "CASER_FUSED_LONG_MAX_BATCH", 1 << 40)
    monkeypatch.setattr(ops.config, "caser_fused", False)
    cz.run(_fused, small, "cuda")
    assert not calls
    monkeypatch.setattr(ops.config, "caser_fused", True)
    cz.run(_fused, small, "cuda")
    assert len(calls) == 1


@pytest.mark.parametrize("c", [0, 1, 2])
def test_encoder_against_the_reference_fixture(monkeypatch, c):
    """The whole network on the GPU: lookup, caser_conv, the two Linears; the project's fixture bar, 1e-4."""
    from test_caser_host import encoder
    calls = _spy(monkeypatch)
    fx = Fixture("caser")
    m = encoder(c).cuda().train()
    x = fx.tensors("in%d" % c, "cuda")
    y = m(x["user"], x["seq"])
    assert len(calls) == 1
    (y * x["up"]).sum().backward()
    out, g = fx.tensors("out%d" % c, "cuda"), fx.tensors("g%d" % c, "cuda")
    assert float((y.detach() - out["seq_output"]).abs().max()) <= 1e-4
    for name, p in m.named_parameters():
        got = p.grad if p.grad is not None else torch.zeros_like(p)
        if got.numel():
            assert float((got - g[name]).abs().max()) <= 1e-4, name


def test_matching_model_on_the_gpu():
    from recbox_amd.rechub.basic.features import SequenceFeature, SparseFeature
    from recbox_amd.rechub.models.matching import Caser
    from conftest import load_params
    from test_caser_host import CASES, N_USERS
    B, L, D, n_h, n_v, n_items = CASES[0]
    fx = Fixture("caser")
    model = Caser(SparseFeature("user_id", N_USERS, D), SequenceFeature("hist_item_id", n_items, D, pooling="concat"), L, n_h, n_v,
                  dropout_prob=0.0)
    load_params(model.encoder, fx["p0"])
    model.cuda()
    x = fx.tensors("in0", "cuda")
    scores = model({"user_id": x["user"], "hist_item_id": x["seq"]})
    want = fx.tensors("out0", "cuda")["seq_output"] @ model.encoder.item_embedding.weight.detach().t()
    assert tuple(scores.shape) == (B, n_items) and float((scores - want).abs().max()) <= 1e-4


def test_report_worst_ratio():
    """Prints the worst err / bar per tensor over this module."""
    fp32_bar.report("caser")
