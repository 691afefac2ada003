"""In-batch band scores (``ops.inbatch_band_scores``, csrc/rbx_inbatch.hip), YoutubeSBC and FaceBookDSSM on the GPU: scores, du,
dv and dw against the float64 restatement of tests/inbatch64.py under the fp32-scaled bar of tests/fp32_bar.py (factor 4, its
floor) over a paired shape grid; column views read in place; a strided scores block through the C ABI; rows with a clamped
norm; run-to-run bits; what the C ABI refuses and where the op sends it; the models against the live reference's fixture; one
graph capture of YoutubeSBC; peak memory against the square the reference materialises."""
import ctypes

import numpy as np
import pytest
import torch

import fp32_bar
import inbatch64

pytestmark = pytest.mark.gpu

R = 16                                                      # rows per workgroup (kIbTile of csrc/rbx_inbatch.hip)
# (B, D, n_neg, weighted): every B of {2, R - 1, R, R + 1, 2 R + 1, 257}, every D of {4, 20, 64, 100, 256, 512}; n_neg of 1, 3,
# B - 1 (below and above the tile), 20 (the halo longer than a tile) and the cap at D = 64 / 256 / 512 (64 / 50 / 22); with and
# without w -- paired, not multiplied.
GRID = [(2, 4, 1, True), (15, 20, 3, False), (16, 64, 15, True), (17, 100, 1, False), (33, 256, 20, True), (257, 512, 22, True),
        (257, 64, 64, False), (257, 256, 50, True), (17, 4, 16, True), (33, 512, 3, False)]
_CACHE = {}


def _refs(case):
    return inbatch64.reference(case), inbatch64.reference(case, torch.float32)


def _case(B, D, n, weighted, seed=11):
    key = (B, D, n, weighted, seed)
    if key not in _CACHE:
        case = inbatch64.make_case(seed, B, D, n, weighted)
        _CACHE[key] = (case, _refs(case))
    return _CACHE[key]


@pytest.fixture
def fused_only(monkeypatch):
    from recbox_amd import ops
    monkeypatch.setattr(ops.config, "inbatch_fused", True)
    monkeypatch.setattr(ops, "inbatch_band_scores_torch", lambda *a, **k: pytest.fail("the fused band op did not run"))


def _assert_all(tag, got, refs, case):
    want, ref32 = refs
    for name in inbatch64.names(case):
        fp32_bar.assert_bar("%s %s" % (name, tag), got[name], want[name], ref32[name])


@pytest.mark.parametrize("shape", GRID, ids=lambda s: "B%d-D%d-n%d-w%d" % s)
def test_op_matches_float64_under_the_fp32_bar(shape, fused_only):
    from recbox_amd import ops
    case, refs = _case(*shape)
    _assert_all(str(shape), inbatch64.run(ops.inbatch_band_scores, case, "cuda"), refs, case)
    fp32_bar.report("inbatch %s" % (shape,))


def test_grid_keeps_every_listed_value():
    from recbox_amd import ops
    assert {s[0] for s in GRID} == {2, R - 1, R, R + 1, 2 * R + 1, 257} and {s[1] for s in GRID} == {4, 20, 64, 100, 256, 512}
    assert {s[2] for s in GRID} >= {1, 3} and {s[3] for s in GRID} == {True, False}
    assert any(s[2] == s[0] - 1 and s[2] < R for s in GRID) and any(s[2] == s[0] - 1 and s[2] >= R for s in GRID)
    assert any(R < s[2] < ops.inbatch_band_max_neg(s[1]) for s in GRID)
    for D in (64, 256, 512):
        assert any(s[1] == D and s[2] == ops.inbatch_band_max_neg(D) for s in GRID), D


def test_u_and_v_are_read_as_column_views_of_a_wider_block(fused_only):
    from recbox_amd import ops
    case, refs = _case(33, 256, 20, True)
    wide_u = torch.full((33, 256 + 24), 7.0, device="cuda")
    wide_v = torch.full((33, 256 + 8), -5.0, device="cuda")
    wide_u[:, 8:264] = case["u"].cuda()
    wide_v[:, 4:260] = case["v"].cuda()
    wide_u.requires_grad_()
    wide_v.requires_grad_()
    for view in (wide_u[:, 8:264], wide_v[:, 4:260]):
        assert ops._inbatch_rows(view).data_ptr() == view.data_ptr()              # no copy is made
    got = inbatch64.run(ops.inbatch_band_scores, case, "cuda", u=(wide_u[:, 8:264], wide_u), v=(wide_v[:, 4:260], wide_v))
    assert float(got["du"][:, :8].abs().max()) == 0.0 and float(got["du"][:, 264:].abs().max()) == 0.0
    assert float(got["dv"][:, :4].abs().max()) == 0.0 and float(got["dv"][:, 260:].abs().max()) == 0.0
    got["du"], got["dv"] = got["du"][:, 8:264], got["dv"][:, 4:260]
    _assert_all("views", got, refs, case)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def test_scores_are_written_with_a_row_stride_and_nothing_else_is_touched():
    from recbox_amd import _lib
    case, refs = _case(33, 256, 20, True)
    B, D, n = case["dims"]
    u, v, w = case["u"].cuda(), case["v"].cuda(), case["w"].cuda()
    block = torch.full((B, n + 1 + 7), -3.0, device="cuda")
    ru, rv = torch.empty(B, device="cuda"), torch.empty(B, device="cuda")
    rc = _lib.lib.rbx_inbatch_band_fwd(u.data_ptr(), D, v.data_ptr(), D, w.data_ptr(), B, D, n, 1e-8, 1.0 / case["temperature"],
                                       _lib.RBX_F32, block.data_ptr() + 2 * 4, block.stride(0), ru.data_ptr(), rv.data_ptr(), _stream())
    assert rc == _lib.RBX_OK, _lib.last_error()
    torch.cuda.synchronize()
    assert bool((block[:, :2] == -3.0).all()) and bool((block[:, 2 + n + 1:] == -3.0).all())
    want, ref32 = refs
    fp32_bar.assert_bar("scores strided", block[:, 2:2 + n + 1], want["scores"], ref32["scores"])
    assert float((ru.cpu().double() - 1.0 / case["u"].double().norm(dim=1)).abs().max()) <= 1e-6 * float(ru.max())
    assert float((rv.cpu().double() - 1.0 / case["v"].double().norm(dim=1)).abs().max()) <= 1e-6 * float(rv.max())


def test_rows_with_a_clamped_norm_give_finite_results_within_the_bar(fused_only):
    from recbox_amd import ops
    case = inbatch64.make_case(13, 33, 64, 3, True)
    case["u"][1] *= 1e-10 / float(case["u"][1].norm())       # far under eps = 1e-8
    case["v"][18] *= 1e-10 / float(case["v"][18].norm())
    case["u"][20] = 0.0
    case["v"][32] = 0.0
    got = inbatch64.run(ops.inbatch_band_scores, case, "cuda")
    for name in inbatch64.names(case):
        assert bool(torch.isfinite(got[name]).all()), name
    _assert_all("clamped", got, _refs(case), case)


def test_two_runs_give_the_same_bits(fused_only):
    from recbox_amd import ops
    case, _ = _case(257, 256, 50, True)
    first, second = inbatch64.run(ops.inbatch_band_scores, case, "cuda"), inbatch64.run(ops.inbatch_band_scores, case, "cuda")
    for name in inbatch64.names(case):
        assert torch.equal(first[name], second[name]), name


class _NodeGuard(object):
    hits = 0

    @classmethod
    def hit(cls, real, *a):
        cls.hits += 1
        return real(*a)


def test_refused_shapes_are_refused_by_the_c_abi_and_run_the_composition(monkeypatch):
    from recbox_amd import _lib, ops
    monkeypatch.setattr(_NodeGuard, "hits", 0)
    real = ops._InbatchBand.apply
    monkeypatch.setattr(ops._InbatchBand, "apply", lambda *a: _NodeGuard.hit(real, *a))
    for B, D, n in ((9, 6, 3), (9, 516, 3), (80, 64, 65), (40, 512, 23), (8, 64, 8)):
        u, v, w = torch.randn(B, D, device="cuda"), torch.randn(B, D, device="cuda"), torch.rand(B, device="cuda") + 0.1
        out, ru, rv = torch.full((B, n + 1), -3.0, device="cuda"), torch.empty(B, device="cuda"), torch.empty(B, device="cuda")
        du, dv, dw = torch.full((B, D), -3.0, device="cuda"), torch.full((B, D), -3.0, device="cuda"), torch.empty(B, device="cuda")
        rc = _lib.lib.rbx_inbatch_band_fwd(u.data_ptr(), D, v.data_ptr(), D, w.data_ptr(), B, D, n, 1e-8, 1.0, _lib.RBX_F32,
                                           out.data_ptr(), n + 1, ru.data_ptr(), rv.data_ptr(), _stream())
        assert rc == _lib.RBX_ERR_UNSUPPORTED, (B, D, n)
        rc = _lib.lib.rbx_inbatch_band_bwd(out.data_ptr(), n + 1, u.data_ptr(), D, v.data_ptr(), D, w.data_ptr(), ru.data_ptr(),
                                           rv.data_ptr(), B, D, n, 1e-8, 1.0, _lib.RBX_F32, du.data_ptr(), D, dv.data_ptr(), D,
                                           dw.data_ptr(), _stream())
        assert rc == _lib.RBX_ERR_UNSUPPORTED, (B, D, n)
        torch.cuda.synchronize()
        assert bool((out == -3.0).all()) and bool((du == -3.0).all()) and bool((dv == -3.0).all())
        if n >= B:
            with pytest.raises(ValueError):
                ops.inbatch_band_scores(u, v, n, weight=w)
            continue
        case = inbatch64.make_case(5, B, D, n, True)
        _assert_all("refused %s" % ((B, D, n),), inbatch64.run(ops.inbatch_band_scores, case, "cuda"), _refs(case), case)
    assert _NodeGuard.hits == 0


# ---- the models ---------------------------------------------------------------------------------------------------------------
def _float64_step(which, tag):
    """The mirror's CPU route in float64 on the recorded batch: the ``want`` of the gradients' bar."""
    import gen_golden_inbatch as gen
    model, fx = inbatch64.loaded(which, "cpu")
    model.double()
    x = {k: (t.double() if t.is_floating_point() else t) for k, t in fx.tensors("in_%s_%s" % (which, tag)).items()}
    up = {k: t.double() for k, t in fx.tensors("up_%s_%s" % (which, tag)).items()}
    gen.loss(which, gen.outputs(which, model(x)), up).backward()
    return {n: p.grad.detach() for n, p in model.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("which,tag", [("sbc", "full"), ("sbc", "short"), ("fb", "full")])
def test_model_matches_the_reference(which, tag, monkeypatch):
    """Outputs within 1e-4 of the fixture; every parameter gradient within the fp32 bar, with the mirror's float64 CPU route as
    ``want`` and the reference's own fp32 gradients (the fixture) as ``ref32``.  The bias in front of a train-mode BatchNorm has
    the exact gradient 0: its floor is scaled by that Linear's weight gradient (tests/inbatch64.py ``grad_scale``)."""
    from recbox_amd import ops
    model, fx = inbatch64.loaded(which, "cuda")
    with monkeypatch.context() as m:                                            # the float64 CPU route below is the composition
        m.setattr(ops.config, "inbatch_fused", True)
        m.setattr(ops, "inbatch_band_scores_torch", lambda *a, **k: pytest.fail("the fused band op did not run"))
        outs, grads = inbatch64.step(which, model, fx, tag, "cuda")
    for k, t in outs.items():
        err = float((t.double().cpu() - torch.from_numpy(np.asarray(fx["out_%s_%s" % (which, tag)][k])).double()).abs().max())
        print("%s %s %s: max abs err %.3e" % (which, tag, k, err))
        assert err <= 1e-4, (which, tag, k, err)
    want, recorded = _float64_step(which, tag), fx["g_%s_%s" % (which, tag)]
    for name, grad in grads.items():
        w64 = want.get(name, torch.zeros_like(grad, dtype=torch.float64, device="cpu"))
        ref32 = torch.from_numpy(np.asarray(recorded[name]))
        bar, e32, scale = fp32_bar.bar_of(w64, ref32)
        floor_scale = inbatch64.grad_scale(model, name, recorded)
        if floor_scale is not None:
            bar = max(bar, fp32_bar.FLOOR * floor_scale)
        err = float((grad.double().cpu() - w64).abs().max())
        print("%s %s grad %s: err %.3e e32 %.3e scale %.3e bar %.3e" % (which, tag, name, err, e32, scale, bar))
        assert err <= bar, "%s %s grad %s: %.3e > %.3e" % (which, tag, name, err, bar)


def test_short_batch_then_full_batch_on_the_gpu(fused_only):
    model, fx = inbatch64.loaded("sbc", "cuda")
    inbatch64.step("sbc", model, fx, "short", "cuda")
    outs, _ = inbatch64.step("sbc", model, fx, "full", "cuda")
    assert inbatch64.rel_err(outs["scores"], fx["out_sbc_full"]["scores"]) <= 1e-4


def _sbc(batch_size):
    import gen_golden_inbatch as gen
    from recbox_amd.rechub.basic import features
    from recbox_amd.rechub.models import matching
    user = [features.SparseFeature("u%d" % i, vocab_size=v, embed_dim=8) for i, v in enumerate(gen.USER_VOCABS)]
    item = [features.SparseFeature("i%d" % i, vocab_size=v, embed_dim=8) for i, v in enumerate(gen.ITEM_VOCABS)]
    tower = {"dims": [16], "activation": "relu", "dropout": 0.0}
    model = matching.YoutubeSBC(user, item, [features.DenseFeature("sw")], dict(tower), dict(tower), batch_size=batch_size,
                                n_neg=3, temperature=0.5)
    gen.seed_params(model, torch.Generator().manual_seed(7))
    return model


def _step(model, x, up):
    y = model(x)
    (y * up).sum().backward()
    return y


def test_capture_of_the_model_replays_the_eager_bits(monkeypatch, fused_only):
    """Forward + backward of YoutubeSBC (B = 32, towers of 16 columns, n_neg = 3) captured once, replayed twice with new ids and
    sample weights."""
    import gen_golden_inbatch as gen
    from recbox_amd import ops
    monkeypatch.setattr(ops.config, "check_ids", False)                         # the id check reads the device
    B = 32
    eager, graphed = _sbc(B), _sbc(B)
    state = {k: v.clone() for k, v in eager.state_dict().items()}
    for model in (eager, graphed):
        model.cuda().train()
    g = torch.Generator().manual_seed(3)
    batches = [{k: v.cuda() for k, v in gen.inputs("sbc", B, g).items()} for _ in range(2)]
    up = torch.randn(B, 4, generator=g).cuda()
    static = {k: torch.zeros_like(v) if not v.is_floating_point() else torch.ones_like(v) for k, v in batches[0].items()}

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            _step(graphed, static, up)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for p in graphed.parameters():
        p.grad = None
    graphed.load_state_dict(state, strict=True)                                 # the warm-up moved the BatchNorm statistics
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = _step(graphed, static, up)
    for batch in batches:
        for p in eager.parameters():
            p.grad = None
        want = _step(eager, batch, up).detach()
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


def test_peak_memory_stays_far_below_the_square(fused_only):
    from recbox_amd import ops
    B, D, n = 2048, 64, 3
    case = inbatch64.make_case(1, B, D, n, True)
    u, v, w = case["u"].cuda().requires_grad_(), case["v"].cuda().requires_grad_(), case["w"].cuda().requires_grad_()
    g = case["g"].cuda()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = ops.inbatch_band_scores(u, v, n, weight=w, temperature=0.5)
    out.backward(g)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print("peak bytes over forward + backward: %d (the [B, B, D] broadcast: %d)" % (peak, B * B * D * 4))
    assert peak < B * B * D * 4 // 16


def test_a_short_batch_inside_the_band_runs_the_kernel_and_matches_the_cpu_route(fused_only):
    """b + n_neg <= batch_size: the short batch is the band op's (i + k) mod b."""
    import gen_golden_inbatch as gen
    on_gpu, on_cpu = _sbc(12), _sbc(12)
    on_gpu.cuda().train()
    on_cpu.train()
    x = gen.inputs("sbc", 9, torch.Generator().manual_seed(5))
    with torch.no_grad():
        got = on_gpu({k: v.cuda() for k, v in x.items()})
        u, v = on_cpu.user_tower(x), on_cpu.item_tower(x)
    case = {"u": u, "v": v, "w": x["sw"], "n_neg": 3, "temperature": 0.5, "g": torch.zeros(9, 4)}
    assert tuple(got.shape) == (9, 4) and inbatch64.rel_err(got, inbatch64.literal(case)) <= 1e-4


def test_bpr_loss_on_the_gpu_matches_the_reference():
    from conftest import Fixture
    from recbox_amd.rechub.basic.loss_func import BPRLoss, HingeLoss
    fx = Fixture("rechub_inbatch")
    t = fx.tensors("loss", "cuda")
    pos, neg = t["pos"].clone().requires_grad_(), t["neg"][:, 0].clone().requires_grad_()
    loss = BPRLoss()(pos, neg)
    loss.backward()
    assert loss.dim() == 0 and inbatch64.rel_err(loss, fx["loss"]["bpr_pairs"]) <= 1e-5
    p64, n64 = t["pos"].double().cpu().requires_grad_(), t["neg"][:, 0].double().cpu().requires_grad_()
    torch.mean(-torch.nn.functional.logsigmoid(p64 - n64)).backward()
    assert inbatch64.rel_err(pos.grad, p64.grad) <= 1e-5 and inbatch64.rel_err(neg.grad, n64.grad) <= 1e-5
    assert inbatch64.rel_err(BPRLoss()(t["pos"].view(-1, 1), t["neg"]), fx["loss"]["bpr_rows"]) <= 1e-5
    assert inbatch64.rel_err(HingeLoss()(t["pos"], t["neg"]), fx["loss"]["hinge"]) <= 1e-5
