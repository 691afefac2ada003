"""The fused GRU on the HIP path (csrc/rbx_gru.hip: ops.gru, the GRU layer, the GRU4Rec / NARM mirrors) against the restatement
of tests/gru64.py in float64 on the CPU, within the project's absolute 1e-4.  Every float64 comparison also runs the fp32
step-loop composition (ops.gru_torch) on the GPU through the same asserts, so an input on which fp32 itself misses the bar
shows as that.  Inputs: x ~ N(0, 1), weights and biases ~ U(-1/sqrt(H), 1/sqrt(H)), lengths uniform in 0..L, upstream gradients
on out and h_n ~ N(0, 1) / sqrt(B L) so that the weight-gradient sums stay O(1)."""
import pytest
import torch

import gru64
from conftest import Fixture, assert_close, assert_grads_close

pytestmark = pytest.mark.gpu
TOL = 1e-4
# (L, I, H): one step; H = 16 (one wavefront); H = 64 (four) at L = 50 and 200; NARM's H = 100 (seven wavefronts, the last one
# a quarter full; I = 50 is no multiple of 4); H = 20 (a partial second wavefront); H = 4 (the floor); H = 128 (the top: eight
# wavefronts, the 32-k-step register layout); H = 96
SHAPES = [(1, 16, 16), (7, 16, 16), (50, 64, 64), (200, 64, 64), (20, 50, 100), (33, 20, 20), (9, 8, 4), (50, 128, 128),
          (12, 32, 96)]
BATCHES = [37, 301]
NAMES = ("out", "h_n", "dx", "dW_ih", "dW_hh", "db_ih", "db_hh", "dh0")


def _inputs(B, L, I, H, seed=0, layers=1):
    g = torch.Generator().manual_seed(100000 * L + 1000 * I + 10 * H + B + seed)
    bound = 1.0 / H ** 0.5

    def uni(*shape):
        return (torch.rand(*shape, generator=g) * 2 - 1) * bound
    params = []
    for k in range(layers):
        params.append([uni(3 * H, I if k == 0 else H), uni(3 * H, H), uni(3 * H), uni(3 * H)])
    return {"x": torch.randn(B, L, I, generator=g), "params": params, "h0": torch.randn(layers, B, H, generator=g),
            "lengths": torch.randint(0, L + 1, (B,), generator=g),
            "up_out": torch.randn(B, L, H, generator=g) / (B * L) ** 0.5,
            "up_hn": torch.randn(layers, B, H, generator=g) / (B * L) ** 0.5}


def _fused(x, layer, h0, lengths):
    from recbox_amd import ops
    return ops.gru(x, layer[0], layer[1], layer[2], layer[3], h0, lengths)


def _composition(x, layer, h0, lengths):
    from recbox_amd import ops
    return ops.gru_torch(x, layer[0], layer[1], layer[2], layer[3], h0, lengths)


def _restatement(x, layer, h0, lengths):
    return gru64.gru_layer(x, layer[0], layer[1], layer[2], layer[3], h0, lengths)


def _run(fn, inp, device, dtype, bias=True, h0=True, lengths=True, use=("out", "h_n")):
    """One layer stack through ``fn``; returns (out, h_n, dx, then per layer dW_ih, dW_hh, db_ih, db_hh, then dh0)."""
    def leaf(t):
        return t.detach().to(device=device, dtype=dtype).requires_grad_(True)
    x = leaf(inp["x"])
    params = [[leaf(p) if (i < 2 or bias) else None for i, p in enumerate(layer)] for layer in inp["params"]]
    h0s = leaf(inp["h0"]) if h0 else None
    lens = inp["lengths"].to(device) if lengths else None
    cur, finals = x, []
    for k, layer in enumerate(params):
        cur, h = fn(cur, layer, h0s[k] if h0s is not None else None, lens)
        finals.append(h)
    hn = torch.stack(finals, dim=0)
    loss = 0
    if "out" in use:
        loss = loss + (cur * inp["up_out"].to(device=device, dtype=cur.dtype)).sum()
    if "h_n" in use:
        loss = loss + (hn * inp["up_hn"].to(device=device, dtype=hn.dtype)).sum()
    loss.backward()
    res = [cur.detach(), hn.detach(), x.grad]
    for layer in params:
        res += [p.grad if p is not None else None for p in layer]
    res.append(h0s.grad if h0s is not None else None)
    return res


def _names(layers):
    names = ["out", "h_n", "dx"]
    for k in range(layers):
        names += ["dW_ih_l%d" % k, "dW_hh_l%d" % k, "db_ih_l%d" % k, "db_hh_l%d" % k]
    return names + ["dh0"]


def _compare(inp, tag, fns=(("composition", _composition), ("fused", _fused)), **form):
    want = _run(_restatement, inp, "cpu", torch.float64, **form)
    for name, fn in fns:
        got = _run(fn, inp, "cuda", torch.float32, **form)
        for what, a, b in zip(_names(len(inp["params"])), got, want):
            assert (a is None) == (b is None), "%s %s" % (name, what)
            if b is not None:
                assert_close(a, b, TOL, "%s %s %s" % (name, what, tag))


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("L,I,H", SHAPES)
def test_against_float64(L, I, H, B):
    """Bias, h0 and lengths all given; a shape the gate refuses runs the composition under ``ops.gru`` and still passes."""
    from recbox_amd import ops
    assert ops.gru_supported(H, L)                            # the whole list is inside the shipped range (4 .. 128)
    _compare(_inputs(B, L, I, H), "B=%d L=%d I=%d H=%d" % (B, L, I, H))


def test_fused_op_runs_the_kernels(monkeypatch):
    """``ops.gru`` on a supported shape enters rbx_gru_fwd / rbx_gru_bwd; with the switch off, or H = 6, it does not."""
    from recbox_amd import ops
    calls = []
    fwd = ops.lib.rbx_gru_fwd

    class Spy(object):
        def rbx_gru_fwd(self, *a):
            calls.append("fwd")
            return fwd(*a)

        def __getattr__(self, name):
            return getattr(ops._lib.lib, name)
    monkeypatch.setattr(ops, "lib", Spy())
    inp = _inputs(37, 7, 16, 16, seed=1)
    _run(_fused, inp, "cuda", torch.float32)
    assert calls == ["fwd"]
    monkeypatch.setattr(ops.config, "gru_fused", False)
    _run(_fused, inp, "cuda", torch.float32)
    assert calls == ["fwd"]
    monkeypatch.setattr(ops.config, "gru_fused", True)
    assert not ops.gru_supported(6, 7)
    _compare(_inputs(37, 7, 10, 6, seed=1), "refused H=6", fns=(("refused shape", _fused),))
    assert calls == ["fwd"]
    x = inp["x"].cuda()
    p = [t.cuda() for t in inp["params"][0]]
    view = torch.randn(37, 7, 32, device="cuda")[:, :, :16]                   # an oddly strided view: the composition
    ops.gru(view, p[0], p[1])
    ops.gru(x.double(), p[0], p[1])                                           # float64: the composition
    assert calls == ["fwd"]


def test_single_sample():
    _compare(_inputs(1, 7, 16, 16, seed=2), "B=1")
    _compare(_inputs(1, 20, 50, 100, seed=2), "B=1 H=100")


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("h0", [True, False])
@pytest.mark.parametrize("lengths", [True, False])
def test_forms(bias, h0, lengths):
    _compare(_inputs(37, 7, 16, 16, seed=3), "bias=%s h0=%s lengths=%s" % (bias, h0, lengths), bias=bias, h0=h0, lengths=lengths)
    _compare(_inputs(37, 20, 50, 100, seed=3), "H=100 bias=%s h0=%s lengths=%s" % (bias, h0, lengths), bias=bias, h0=h0,
             lengths=lengths)


@pytest.mark.parametrize("use", [("h_n",), ("out",)])
def test_only_one_output_used(use):
    """GRU4Rec reads h_n alone, a sequence model out alone: the unused output's gradient is absent, not a zero tensor."""
    _compare(_inputs(37, 7, 16, 16, seed=4), "use=%s" % (use,), use=use)
    _compare(_inputs(301, 50, 64, 64, seed=4), "use=%s H=64" % (use,), use=use, bias=False, h0=False, lengths=False)


@pytest.mark.parametrize("L,I,H", [(7, 16, 16), (20, 50, 100)])
def test_two_stacked_layers(L, I, H):
    _compare(_inputs(37, L, I, H, seed=5, layers=2), "2 layers H=%d" % H)


def test_all_lengths_zero():
    inp = _inputs(37, 7, 16, 16, seed=6)
    inp["lengths"] = torch.zeros(37, dtype=torch.long)
    _compare(inp, "lengths all 0")
    got = _run(_fused, inp, "cuda", torch.float32)
    assert (got[0] == 0).all() and torch.equal(got[1][0].cpu(), inp["h0"][0]) and (got[2] == 0).all()
    assert torch.equal(got[7].cpu(), inp["up_hn"])            # dh0 = the upstream gradient of h_n, passed through unchanged


def test_lengths_0_1_and_L_share_a_tile():
    inp = _inputs(37, 9, 16, 20, seed=7)
    inp["lengths"] = torch.tensor(([0, 1, 9, 1, 0, 9, 9, 0, 1, 4] * 4)[:37])
    assert set(inp["lengths"][:16].tolist()) >= {0, 1, 9}    # one workgroup's 16 samples mix all three
    _compare(inp, "lengths 0 / 1 / L in one tile")
    inp["lengths"] = inp["lengths"].int()                     # int32 lengths read the same
    _compare(inp, "int32 lengths", fns=(("fused", _fused),))


def test_masked_positions_are_exactly_zero():
    inp = _inputs(301, 33, 20, 20, seed=8)
    got = _run(_fused, inp, "cuda", torch.float32)
    dead = (torch.arange(33).unsqueeze(0) >= inp["lengths"].unsqueeze(1)).cuda()
    assert dead.any() and (~dead).any()
    assert (got[0][dead] == 0).all() and (got[2][dead] == 0).all()            # out, and d_gi's effect on dx
    assert (got[0][~dead] != 0).any() and (got[2][~dead] != 0).any()


@pytest.mark.parametrize("L,I,H", [(50, 64, 64), (20, 50, 100), (50, 128, 128)])
def test_determinism(L, I, H):
    inp = _inputs(301, L, I, H, seed=9)
    first = _run(_fused, inp, "cuda", torch.float32)
    second = _run(_fused, inp, "cuda", torch.float32)
    for a, b in zip(first, second):
        assert torch.equal(a, b)


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


def test_graph_capture_replays_the_eager_bits():
    from recbox_amd import ops
    B, L, I, H = 301, 20, 50, 100
    inp = _inputs(B, L, I, H, seed=10)
    eager = _run(_fused, inp, "cuda", torch.float32)
    xs = torch.zeros(B, L, I, device="cuda").requires_grad_(True)
    ps = [p.cuda().requires_grad_(True) for p in inp["params"][0]]
    h0 = inp["h0"][0].cuda().requires_grad_(True)
    lens = torch.full((B,), L, device="cuda")
    uo, uh = inp["up_out"].cuda(), inp["up_hn"][0].cuda()

    def step():
        out, hn = ops.gru(xs, ps[0], ps[1], ps[2], ps[3], h0, lens)
        ((out * uo).sum() + (hn * uh).sum()).backward()
        return out, hn

    def zero():
        for t in [xs, h0] + ps:
            t.grad = None
    graph, (out, hn) = _capture(step, zero)
    with torch.no_grad():
        xs.copy_(inp["x"].cuda())
        lens.copy_(inp["lengths"].cuda())
    graph.replay()
    torch.cuda.synchronize()
    got = [out.detach(), hn.detach().unsqueeze(0), xs.grad] + [p.grad for p in ps] + [h0.grad.unsqueeze(0)]
    for what, a, b in zip(_names(1), got, eager):
        assert torch.equal(a, b), what


# ---- models -----------------------------------------------------------------------------------------------------------------
def _mirror(tag):
    from test_gru_host import _mirror as build
    return build(tag)


def _model_step(tag, model, x):
    if tag == "narm":
        y = model({"session": x["session"]})
    else:
        y = model(x)
    y.sum().backward()
    return y


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("tag", ["gru4rec", "narm"])
def test_models_match_the_reference_fixture(tag, fused, monkeypatch):
    from recbox_amd import ops
    monkeypatch.setattr(ops.config, "gru_fused", fused)
    fx = Fixture("rechub_session")
    model = _mirror(tag)
    model.load_state_dict(fx.tensors("p_" + tag), strict=True)
    model = model.cuda().train()
    x = fx.tensors("in", device="cuda")
    if tag == "gru4rec":
        model.mode = "user"
        assert_close(model(x), fx["out_gru4rec"]["user"], TOL, "user")
        model.load_state_dict(fx.tensors("p_" + tag), strict=True)          # (the BatchNorm running statistics moved)
        model.mode = None
    y = _model_step(tag, model, x)
    assert_close(y, fx["out_" + tag]["y" if tag == "gru4rec" else "s"], TOL, "output " + tag)
    assert_grads_close(model, fx["g_" + tag], TOL)


def test_narm_step_is_capturable_and_replays_the_eager_bits(monkeypatch):
    """NARM's forward + backward as one graph: the lengths are counted on the device, nothing is packed or copied to the host
    (narm.py:49-50 cannot be captured)."""
    from recbox_amd import ops
    monkeypatch.setattr(ops.config, "check_ids", False)      # the id check of the lookup reads a status word on the host
    fx = Fixture("rechub_session")
    ids = fx.tensors("in", device="cuda")["session"]

    def make():
        m = _mirror("narm")
        m.load_state_dict(fx.tensors("p_narm"), strict=True)
        return m.cuda().train()
    eager = make()
    y_e = _model_step("narm", eager, {"session": ids})
    model = make()
    buf = torch.ones_like(ids)

    def step():
        return _model_step("narm", model, {"session": buf})

    def zero():
        for p in model.parameters():
            p.grad = None
    graph, y = _capture(step, zero)
    buf.copy_(ids)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y.detach(), y_e.detach())
    for (n, a), (_, b) in zip(model.named_parameters(), eager.named_parameters()):
        assert torch.equal(a.grad, b.grad), n


def test_compat_resolves_the_models_to_the_mirrors():
    import importlib
    from recbox_amd import compat
    from recbox_amd.rechub.models import matching
    report = compat.install(prefixes=("torch_rechub",))
    try:
        mod = importlib.import_module("torch_rechub.models.matching")
        assert mod.GRU4Rec is matching.GRU4Rec and mod.NARM is matching.NARM
    finally:
        compat.uninstall(report)
