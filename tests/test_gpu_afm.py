"""AFM's fused pair-attention pooling on the HIP path (csrc/rbx_afm.hip: ops.afm_pool, recbole.context_aware.AFMInteraction,
rechub's AFM) against the float64 restatement of tests/afm64.py, every tensor under tests/fp32_bar.py's bar with factor 4, and
against tests/golden/afm.npz (recorded from the live reference by tests/gen_golden_afm.py).  Inputs: afm64.make_case, whose
pre-activations are exact in fp32 in any order, so no ReLU unit flips between the kernels and the restatement.

Batch sizes: 1; 37 (no multiple of the 4 samples a workgroup takes per trip); 301; and 2051 -- the launch has at most 512
workgroups of 4 wavefronts, one sample per wavefront and trip, so 2051 samples take the grid-stride loop into a second trip,
and the backward leaves 2048 rows of partial (dW, dh) that the tail adds in chunks of 16 rows per lane."""
import functools

import pytest
import torch

import afm64
import fp32_bar
from conftest import Fixture

pytestmark = pytest.mark.gpu
# (F, D, A): P = 1; small P; P = 10 below one pair tile; P = 21 crossing a tile; D and A no multiples of 16; P = 325; P = 741;
# the widest D and A; A = 33 padded to 64
SHAPES = [(2, 4, 1), (3, 8, 4), (5, 8, 25), (7, 16, 32), (6, 20, 7), (26, 16, 25), (39, 16, 32), (10, 64, 64), (12, 32, 33)]
SECOND_TRIP = 2051


@functools.lru_cache(maxsize=None)
def _case(B, F, D, A, seed=0, h_scale=0.1, up_scale=1.0, nonpos=False):
    return afm64.make_case(B, F, D, A, seed, h_scale, up_scale, nonpos)


@functools.lru_cache(maxsize=None)
def _refs(B, F, D, A, seed=0, h_scale=0.1, up_scale=1.0, nonpos=False):
    case = _case(B, F, D, A, seed, h_scale, up_scale, nonpos)
    return afm64.reference(case), afm64.reference(case, dtype=torch.float32)


def _fused(*a):
    from recbox_amd import ops
    return ops.afm_pool(*a)


def _composition(*a):
    from recbox_amd import ops
    return ops.afm_pool_torch(*a)


def _check(got, refs, what):
    want, ref32 = refs
    for n in afm64.NAMES:
        fp32_bar.assert_bar("%s %s" % (n, what), got[n], want[n], ref32[n])


def _same_bits(a, b, what=""):
    for n in afm64.NAMES:
        if a[n] is None or b[n] is None:
            assert a[n] is None and b[n] is None, n
        else:
            assert torch.equal(a[n], b[n]), "%s %s" % (what, n)


def _spy(monkeypatch):
    """Counts the calls that reach rbx_afm_fwd."""
    from recbox_amd import ops
    calls = []
    fwd = ops.lib.rbx_afm_fwd
    monkeypatch.setattr(ops.lib, "rbx_afm_fwd", lambda *a: (calls.append(1), fwd(*a))[1])
    return calls


def test_graph_capture_replays_the_eager_bits():
    """Forward + backward of (5, 8, 25) at B = 37 captured once with torch.cuda.graph: the replay equals the eager run bit for
    bit (no allocation, read-back or stream switch inside the C calls)."""
    case = _case(37, 5, 8, 25)
    eager = afm64.run(_fused, case, "cuda")
    x = case["x"].cuda().requires_grad_()
    w = case["w"].cuda().requires_grad_()
    h = case["h"].cuda().requires_grad_()
    up = case["up"].cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                      # warm up off the default stream, as capture requires
        out, _ = _fused(x, w, h, True)
        torch.autograd.grad((out * up).sum(), (x, w, h))
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, attn = _fused(x, w, h, True)
        dx, dw, dh = torch.autograd.grad((out * up).sum(), (x, w, h))
    for t in (out, attn, dx, dw, dh):
        t.detach().zero_()
    graph.replay()
    torch.cuda.synchronize()
    got = {"out": out.detach(), "attn": attn, "dx": dx, "dW": dw, "dh": dh}
    _same_bits(got, eager, "replay")


@pytest.mark.parametrize("B", [1, 37])
@pytest.mark.parametrize("F,D,A", SHAPES)
def test_every_shape_against_float64(monkeypatch, F, D, A, B):
    calls = _spy(monkeypatch)
    case = _case(B, F, D, A)
    got = afm64.run(_fused, case, "cuda")
    assert len(calls) == 1
    _check(got, _refs(B, F, D, A), "F%d D%d A%d B%d" % (F, D, A, B))
    if F == 2:                                                         # one pair: the softmax is exactly 1 and carries no gradient
        assert torch.equal(got["attn"], torch.ones_like(got["attn"]))
        assert not got["dW"].any() and not got["dh"].any()


@pytest.mark.parametrize("F,D,A", [(5, 8, 25), (26, 16, 25), (12, 32, 33)])
def test_batch_301(F, D, A):
    _check(afm64.run(_fused, _case(301, F, D, A), "cuda"), _refs(301, F, D, A), "F%d D%d A%d B301" % (F, D, A))


@pytest.mark.parametrize("F,D,A", [(5, 8, 25), (7, 16, 32)])
def test_second_trip_and_more_than_one_chunk_of_partials(F, D, A):
    B = SECOND_TRIP
    from recbox_amd import ops
    rows = ops.lib.rbx_afm_bwd_workspace_size(B, F, D, A) // (4 * (A * D + A))
    assert rows == 2048 and B > rows                                   # a second trip; 128 rows per lane of the tail
    _check(afm64.run(_fused, _case(B, F, D, A), "cuda"), _refs(B, F, D, A), "F%d D%d A%d B%d" % (F, D, A, B))


def test_small_upstream_gradient():
    """Upstream gradients scaled by 1e-3: the bar scales with them (an absolute 1e-4 would pass zeros)."""
    key = (37, 7, 16, 32, 1, 0.1, 1e-3)
    _check(afm64.run(_fused, _case(*key), "cuda"), _refs(*key), "up1e-3")


def test_all_units_closed():
    """x >= 0 and W = -|W|: every pre-activation <= 0 (exact zeros among them), so every logit is 0: attn is exactly 1 / P, out
    the plain mean of the pairs, dW and dh exactly zero (strict pre > 0), dx against float64."""
    key = (37, 7, 16, 32, 2, 0.1, 1.0, True)
    case = _case(*key)
    assert case["zeros"] > 0
    got = afm64.run(_fused, case, "cuda")
    assert torch.equal(got["attn"], torch.full_like(got["attn"], 1.0) / 21.0)
    assert not got["dW"].any() and not got["dh"].any()
    _check(got, _refs(*key), "closed")


def test_large_logits_stay_finite():
    key = (37, 7, 16, 32, 3, 4.0)
    want, _ = _refs(*key)
    x, w, h = (_case(*key)[k].double() for k in ("x", "w", "h"))
    s = torch.relu((x[:, :1] * x[:, 1:2]) @ w.t()) @ h
    assert float(s.abs().max()) > 40                                   # logits of this magnitude (spread about 90) are in play
    got = afm64.run(_fused, _case(*key), "cuda")
    for n in afm64.NAMES:
        assert torch.isfinite(got[n]).all(), n
    _check(got, _refs(*key), "large logits")


def test_strided_x_and_noncontiguous_dout(monkeypatch):
    calls = _spy(monkeypatch)
    B, F, D, A = 37, 7, 16, 32
    case = _case(B, F, D, A)
    wide = torch.zeros(B, F, D + 8, device="cuda")
    wide[:, :, 4:4 + D] = case["x"].cuda()
    wide.requires_grad_()
    up = torch.zeros(D, B, device="cuda")
    up.copy_(case["up"].cuda().t())
    got = afm64.run(_fused, case, "cuda", x=(wide[:, :, 4:4 + D], wide), up=up.t())
    assert len(calls) == 1
    got["dx"] = got["dx"][:, :, 4:4 + D]
    _check(got, _refs(B, F, D, A), "strided")
    assert not wide.grad[:, :, :4].any() and not wide.grad[:, :, 4 + D:].any()


@pytest.mark.parametrize("needs", [(True, False, False), (False, True, False), (False, False, True), (True, True, False),
                                   (False, True, True), (True, False, True)])
def test_needs_input_grad_subsets(needs):
    case = _case(37, 7, 16, 32)
    full = afm64.run(_fused, case, "cuda")
    got = afm64.run(_fused, case, "cuda", needs=needs)
    for n, need in zip(("dx", "dW", "dh"), needs):
        if need:
            assert torch.equal(got[n], full[n]), n
        else:
            assert got[n] is None, n


def test_want_attn_off_gives_the_same_out_bits():
    case = _case(37, 26, 16, 25)
    on = afm64.run(_fused, case, "cuda", want_attn=True)
    off = afm64.run(_fused, case, "cuda", want_attn=False)
    assert off["attn"] is None
    for n in ("out", "dx", "dW", "dh"):
        assert torch.equal(on[n], off[n]), n


def test_two_runs_give_equal_bits():
    case = _case(301, 26, 16, 25)
    _same_bits(afm64.run(_fused, case, "cuda"), afm64.run(_fused, case, "cuda"), "rerun")


def test_switch_off_and_refused_shapes_run_the_composition(monkeypatch):
    from recbox_amd import ops
    calls = _spy(monkeypatch)
    case = _case(37, 5, 8, 25)
    monkeypatch.setattr(ops.config, "afm_fused", False)
    _same_bits(afm64.run(_fused, case, "cuda"), afm64.run(_composition, case, "cuda"), "switch off")
    monkeypatch.setattr(ops.config, "afm_fused", True)
    for F, D in ((5, 6), (40, 8)):
        g = torch.Generator().manual_seed(F)
        odd = {"x": torch.randn(9, F, D, generator=g), "w": torch.randn(5, D, generator=g), "h": torch.randn(5, generator=g),
               "up": torch.randn(9, D, generator=g)}
        _same_bits(afm64.run(_fused, odd, "cuda"), afm64.run(_composition, odd, "cuda"), "refused F%d D%d" % (F, D))
    assert not calls


@pytest.mark.parametrize("c", [0, 1])
def test_interaction_against_the_reference_fixture(c):
    from recbox_amd.recbole.context_aware import AFMInteraction
    fx = Fixture("afm")
    x = fx.tensors("in%d" % c, "cuda")
    B, F, D = x["x"].shape
    A = fx["p%d" % c]["attlayer.h"].shape[0]
    m = AFMInteraction(F, D, A, 0.0)
    m.load_state_dict(fx.tensors("p%d" % c), strict=True)
    m.cuda().train()
    leaf = x["x"].clone().requires_grad_()
    y = m(leaf)
    (y * x["up"]).sum().backward()
    out, g = fx.tensors("out%d" % c, "cuda"), fx.tensors("g%d" % c, "cuda")
    assert float((y - out["y"]).abs().max()) <= 1e-4
    assert float((m.attention(leaf) - out["att"]).abs().max()) <= 1e-4
    assert float((leaf.grad - g["x"]).abs().max()) <= 1e-4
    for name, p in m.named_parameters():
        assert float((p.grad - g[name]).abs().max()) <= 1e-4, name


def test_model_against_the_reference_fixture():
    """rechub-style AFM whose tables hold the fixture's x (row b of table f = x[b, f]) and whose interaction holds the fixture's
    parameters: the logit is the first-order term plus the recorded afm_layer output."""
    from recbox_amd.rechub.basic.features import SparseFeature
    from recbox_amd.rechub.models.ranking import AFM
    fx = Fixture("afm")
    x = fx.tensors("in0")["x"]
    B, F, D = x.shape
    A = fx["p0"]["attlayer.h"].shape[0]
    torch.manual_seed(5)
    model = AFM([SparseFeature("s%d" % f, vocab_size=B, embed_dim=D) for f in range(F)], attention_size=A, dropout_prob=0.0)
    model.interaction.load_state_dict(fx.tensors("p0"), strict=True)
    with torch.no_grad():
        for f in range(F):
            model.embedding.embed_dict["s%d" % f].weight.copy_(x[:, f])
    lin = model.linear.fc
    want = torch.sigmoid(x.flatten(1).double() @ lin.weight.detach().double().t() + lin.bias.detach().double()
                         + fx.tensors("out0")["y"].double()).squeeze(1)
    model.cuda().train()
    y = model({"s%d" % f: torch.arange(B, device="cuda") for f in range(F)})
    assert float((y.double().cpu() - want).abs().max()) <= 1e-4
    y.sum().backward()
    for p in model.parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all()


def test_report_worst_ratio():
    """Prints the worst err / bar per tensor over this module (profiles/afm/INDEX.md quotes it)."""
    fp32_bar.report("afm")
