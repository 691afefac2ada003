"""AutoInt's fused interacting layer on the HIP path (csrc/rbx_fieldattn.hip: ops.field_attn, recbole.AutoIntInteraction,
rechub's AutoInt) against the float64 restatement of tests/fieldattn64.py, every tensor under tests/fp32_bar.py's bar with
factor 4 (``ref32`` the fp32 CPU composition), and against tests/golden/autoint.npz (recorded from the live reference by
tests/gen_golden_autoint.py).

A launch has ceil(B / (2 nw)) workgroups (at most 512) of nw <= 4 wavefronts, one sample per wavefront and trip: B = 37 is no
multiple of a workgroup's samples, B = 301 takes every wavefront into a second, partial trip and leaves 152 rows of partial
weight gradients, B = 1200 leaves 600, which the tail adds 16 rows at a time (38 chunks)."""
import functools
import itertools
import math

import pytest
import torch

import fieldattn64 as fa
import fp32_bar
from conftest import Fixture

pytestmark = pytest.mark.gpu
# (F, E, h): the smallest; F below a tile; three heads; F a whole tile; one field past it; one head of width 32; the Criteo
# counts 26 and 39; four heads; the largest F and E with the most heads (width 4)
SHAPES = [(2, 4, 1), (3, 8, 2), (5, 12, 3), (16, 16, 2), (17, 16, 2), (23, 32, 1), (26, 16, 2), (39, 16, 2), (39, 32, 4),
          (48, 32, 8)]
# (residual, relu, biases)
FORMS = [(False, False, True), (True, True, True), (True, False, False), (False, True, False)]
ALL = fa.NAMES + ("attn",)


@pytest.fixture(autouse=True)
def _whole_range(monkeypatch):
    """The default routing sends only the classes measured faster to the kernels; these tests run them over their whole range."""
    from recbox_amd import ops
    monkeypatch.setattr(ops.config, "field_attn_fields", ops.FIELD_ATTN_MAX_FIELDS)
    monkeypatch.setattr(ops.config, "field_attn_dim", ops.FIELD_ATTN_MAX_DIM)


@functools.lru_cache(maxsize=None)
def _case(B, F, E, h, res=False, relu=False, bias=True, p=0.0, seed=0, w_scale=0.6, up_scale=1.0):
    return fa.make_case(B, F, E, h, res, relu, bias, p, seed, w_scale, up_scale)


@functools.lru_cache(maxsize=None)
def _refs(*key):
    case = _case(*key)
    return fa.reference(case), fa.ref32(case)


def _fused(*a):
    from recbox_amd import ops
    return ops.field_attn(*a)


def _composition(*a):
    from recbox_amd import ops
    return ops.field_attn_torch(*a)


def _check(got, refs, what, names=ALL):
    want, ref32 = refs
    for n in names:
        if want[n] is None:
            assert got[n] is None, n
        else:
            fp32_bar.assert_bar("%s %s" % (n, what), got[n], want[n], ref32[n])


def _same_bits(a, b, what="", names=ALL):
    for n in names:
        if a[n] is None or b[n] is None:
            assert a[n] is None and b[n] is None, n
        else:
            assert torch.equal(a[n], b[n]), "%s %s" % (what, n)


def _spy(monkeypatch):
    """Counts the calls that reach rbx_fieldattn_fwd."""
    from recbox_amd import ops
    calls = []
    fwd = ops.lib.rbx_fieldattn_fwd
    monkeypatch.setattr(ops.lib, "rbx_fieldattn_fwd", lambda *a: (calls.append(1), fwd(*a))[1])
    return calls


def test_graph_capture_replays_the_eager_bits():
    """Forward + backward of (7, 16, 2) at B = 37 with residual and relu, captured once with torch.cuda.graph: the replay
    equals the eager run bit for bit (no allocation, read-back or stream switch inside the C calls)."""
    case = _case(37, 7, 16, 2, True, True)
    eager = fa.run(_fused, case, "cuda")
    names = ("x", "in_w", "in_b", "out_w", "out_b", "res")
    t = [case[n].cuda().requires_grad_() for n in names]
    up = case["up"].cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                      # warm up off the default stream, as capture requires
        y, _ = _fused(t[0], t[1], t[2], t[3], t[4], 2, t[5], True, 0.0, None, True)
        torch.autograd.grad((y * up).sum(), t)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y, attn = _fused(t[0], t[1], t[2], t[3], t[4], 2, t[5], True, 0.0, None, True)
        grads = torch.autograd.grad((y * up).sum(), t)
    for g in (y, attn) + tuple(grads):
        g.detach().zero_()
    graph.replay()
    torch.cuda.synchronize()
    got = dict(zip(("dx", "dWin", "dbin", "dWout", "dbout", "dres"), grads), y=y.detach(), attn=attn)
    _same_bits(got, eager, "replay")


@pytest.mark.parametrize("B", [1, 37])
@pytest.mark.parametrize("res,relu,bias", FORMS)
@pytest.mark.parametrize("F,E,h", SHAPES)
def test_every_shape_against_float64(monkeypatch, F, E, h, res, relu, bias, B):
    from recbox_amd import ops
    assert ops.field_attn_supported(F, E, h)
    calls = _spy(monkeypatch)
    key = (B, F, E, h, res, relu, bias)
    got = fa.run(_fused, _case(*key), "cuda")
    assert len(calls) == 1
    _check(got, _refs(*key), "F%d E%d h%d B%d res%d relu%d bias%d" % (F, E, h, B, res, relu, bias))


@pytest.mark.parametrize("F,E,h", [(3, 8, 2), (17, 16, 2), (26, 32, 4)])
def test_batch_301_second_partial_trip(F, E, h):
    from recbox_amd import ops
    key = (301, F, E, h, True, True)
    rows = ops.lib.rbx_fieldattn_bwd_workspace_size(301, F, E, h) // (4 * (4 * E * E + 4 * E))
    assert rows < 301 < 2 * rows                                       # every wavefront a second trip, the last one partial
    _check(fa.run(_fused, _case(*key), "cuda"), _refs(*key), "F%d E%d h%d B301" % (F, E, h))


def test_many_chunks_of_partial_rows():
    from recbox_amd import ops
    key = (1200, 3, 8, 2, True, True)
    rows = ops.lib.rbx_fieldattn_bwd_workspace_size(1200, 3, 8, 2) // (4 * (4 * 64 + 32))
    assert rows == 600                                                 # 38 chunks of 16 rows in the tail
    _check(fa.run(_fused, _case(*key), "cuda"), _refs(*key), "B1200")


def test_small_upstream_gradient():
    """Upstream gradients scaled by 1e-3: the bar scales with them (an absolute 1e-4 would pass zeros)."""
    key = (37, 7, 16, 2, True, True, True, 0.0, 1, 0.6, 1e-3)
    _check(fa.run(_fused, _case(*key), "cuda"), _refs(*key), "up1e-3")


@pytest.mark.parametrize("F,E,h", [(7, 16, 2), (39, 16, 2), (18, 32, 4)])
def test_dropout_equals_the_restatement_under_the_kernels_mask(F, E, h):
    """p = 0.25 with a fixed seed: the fused layer equals the float64 restatement under
    ops.attention_dropout_mask(B h, F, F, p, seed), same bar; the kept fraction of that mask is within 3 sigma of 0.75; attn
    is the pre-dropout probabilities."""
    from recbox_amd import ops
    B, p, seed = 37, 0.25, 20261021
    case = _case(B, F, E, h, True, True, True, p)
    keep = ops.attention_dropout_mask(B * h, F, F, p, seed)
    n = keep.numel()
    assert abs(float(keep.float().mean()) - 0.75) <= 3.0 * math.sqrt(0.75 * 0.25 / n)
    got = fa.run(_fused, case, "cuda", seed=seed)
    want, ref32 = fa.reference(case, keep), fa.ref32(case, keep)
    _check(got, (want, ref32), "dropout F%d E%d h%d" % (F, E, h))
    again = fa.run(_fused, case, "cuda", seed=seed)
    _same_bits(got, again, "same seed")
    other = fa.run(_fused, case, "cuda", seed=seed + 1)
    assert not torch.equal(other["y"], got["y"])


def test_want_attn_rows_sum_to_one_and_leave_y_alone():
    key = (37, 26, 16, 2, True, True)
    on = fa.run(_fused, _case(*key), "cuda", want_attn=True)
    off = fa.run(_fused, _case(*key), "cuda", want_attn=False)
    assert off["attn"] is None
    _same_bits(on, off, "want_attn", fa.NAMES)
    assert tuple(on["attn"].shape) == (37, 2, 26, 26)
    assert float((on["attn"].double().sum(-1) - 1.0).abs().max()) <= 1e-6
    want, ref32 = _refs(*key)
    fp32_bar.assert_bar("attn want_attn", on["attn"], want["attn"], ref32["attn"])


def test_transposed_view_and_noncontiguous_dy_give_the_same_bits(monkeypatch):
    """x as the reference holds it, the [F, B, E] tensor's transpose, and a non-contiguous upstream gradient."""
    calls = _spy(monkeypatch)
    key = (37, 7, 16, 2, True, True)
    case = _case(*key)
    plain = fa.run(_fused, case, "cuda")
    fbe = case["x"].cuda().transpose(0, 1).contiguous().requires_grad_()       # [F, B, E]
    up = torch.zeros(37, 7, 24, device="cuda")
    up[:, :, 4:20] = case["up"].cuda()
    got = fa.run(_fused, case, "cuda", x=(fbe.transpose(0, 1), fbe), up=up[:, :, 4:20])
    assert len(calls) == 2
    got["dx"] = got["dx"].transpose(0, 1)
    _same_bits(got, plain, "views")
    upt = case["up"].cuda().transpose(1, 2).contiguous().transpose(1, 2)        # inner stride F: copied by the op
    _same_bits(fa.run(_fused, case, "cuda", up=upt), plain, "dy with an inner stride")


def test_every_subset_of_needs_input_grad():
    case = _case(9, 5, 8, 2, True, True)
    full = fa.run(_fused, case, "cuda")
    names = ("dx", "dWin", "dbin", "dWout", "dbout", "dres")
    for needs in itertools.product((False, True), repeat=6):
        if not any(needs):
            continue
        got = fa.run(_fused, case, "cuda", needs=needs)
        for n, need in zip(names, needs):
            if need:
                assert torch.equal(got[n], full[n]), (n, needs)
            else:
                assert got[n] is None, (n, needs)


def test_two_runs_give_equal_bits():
    case = _case(301, 26, 32, 4, True, True)
    _same_bits(fa.run(_fused, case, "cuda"), fa.run(_fused, case, "cuda"), "rerun")


def test_large_logits_stay_finite():
    key = (37, 7, 16, 2, False, False, True, 0.0, 0, 6.0)
    _, _, _, q, k, _, _ = fa.forward64(_case(*key))
    assert float((q @ k.transpose(-2, -1)).abs().max()) > 80
    got = fa.run(_fused, _case(*key), "cuda")
    for n in ALL:
        assert got[n] is None or torch.isfinite(got[n]).all(), n
    _check(got, _refs(*key), "large logits")


def test_switch_off_and_refusals_run_the_composition(monkeypatch):
    from recbox_amd import ops
    calls = _spy(monkeypatch)
    case = _case(9, 5, 8, 2, True, True)
    monkeypatch.setattr(ops.config, "field_attn_fused", False)
    _same_bits(fa.run(_fused, case, "cuda"), fa.run(_composition, case, "cuda"), "switch off")
    monkeypatch.setattr(ops.config, "field_attn_fused", True)
    for F, E, h in ((5, 6, 1), (49, 8, 2), (5, 36, 1), (5, 8, 4), (5, 12, 2)):
        assert not ops.field_attn_supported(F, E, h)
        odd = fa.make_case(9, F, E, h, True, True)
        _same_bits(fa.run(_fused, odd, "cuda"), fa.run(_composition, odd, "cuda"), "refused F%d E%d h%d" % (F, E, h))
    wide = torch.zeros(9, 5, 8, 2, device="cuda")                      # an inner stride of 2: an odd layout
    wide[..., 0] = case["x"].cuda()
    leaf = wide.requires_grad_()
    got = fa.run(_fused, case, "cuda", x=(leaf[..., 0], leaf))
    got["dx"] = got["dx"][..., 0]
    _same_bits(got, fa.run(_composition, case, "cuda"), "inner stride")
    half = {k: (v.double() if torch.is_tensor(v) else v) for k, v in case.items()}
    assert fa.run(_fused, half, "cuda")["y"].dtype == torch.float64       # not float32: the composition
    assert not calls
    fa.run(_fused, case, "cuda")
    assert len(calls) == 1


def test_default_gate_sends_the_measured_classes_only(monkeypatch):
    """As shipped: 26 fields x 16 reach the kernels, 39 fields or a width of 32 run the composition."""
    from recbox_amd import ops
    monkeypatch.undo()
    assert (ops.config.field_attn_fields, ops.config.field_attn_dim) == (32, 16)
    calls = _spy(monkeypatch)
    fa.run(_fused, _case(9, 26, 16, 2), "cuda")
    assert len(calls) == 1
    for F, E in ((39, 16), (26, 32)):
        case = _case(9, F, E, 2)
        _same_bits(fa.run(_fused, case, "cuda"), fa.run(_composition, case, "cuda"), "gated F%d E%d" % (F, E))
    assert len(calls) == 1


@pytest.mark.parametrize("c", [0, 1])
def test_interaction_against_the_reference_fixture(monkeypatch, c):
    from recbox_amd.recbole import AutoIntInteraction
    from test_autoint_host import interaction
    calls = _spy(monkeypatch)
    fx = Fixture("autoint")
    m = interaction(c).cuda().train()
    x = fx.tensors("in%d" % c, "cuda")
    assert isinstance(m, AutoIntInteraction)
    leaf = x["x"].clone().requires_grad_()
    y = m(leaf)
    assert len(calls) == m.n_layers
    (y * x["up"]).sum().backward()
    out, g = fx.tensors("out%d" % c, "cuda"), fx.tensors("g%d" % c, "cuda")
    assert float((y - out["y"]).abs().max()) <= 1e-4
    assert float((leaf.grad - g["x"]).abs().max()) <= 1e-4
    for name, p in m.named_parameters():
        assert float((p.grad - g[name]).abs().max()) <= 1e-4, name


def test_model_against_the_reference_fixture():
    """rechub-style AutoInt whose tables hold the fixture's x (row b of table f = x[b, f]) and whose interaction holds the
    fixture's parameters: the logit is the first-order term plus the recorded autoint_layer output."""
    from test_autoint_host import model_and_want
    model, ids, want = model_and_want("cuda")
    model.cuda().train()
    y = model(ids)
    assert float((y.double().cpu() - want).abs().max()) <= 1e-4
    y.sum().backward()
    for p in model.parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all()


def test_report_worst_ratio():
    """Prints the worst err / bar per tensor over this module (profiles/autoint/INDEX.md quotes it)."""
    fp32_bar.report("autoint")
