"""In-batch band scores (``ops.inbatch_band_scores``, csrc/rbx_inbatch.hip), YoutubeSBC, FaceBookDSSM and the pair-wise losses,
the parts that need no GPU: the float64 restatement of tests/inbatch64.py against the reference model's literal expression; the
composition against the restatement; both mirrors on the CPU route against the live reference's fixture
(tests/golden/rechub_inbatch.npz, written by tests/gen_golden_inbatch.py) with its ordered state_dict keys, the short batch and
both modes; the losses; the compat paths; the C ABI's entries and their refusals."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest
import torch

import fp32_bar
import inbatch64
from conftest import Fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["rbx_inbatch_band_fwd", "rbx_inbatch_band_bwd"]
OTHER = ["rbx_inbatch_band_supported", "rbx_inbatch_band_max_neg"]
LITERAL = [(7, 5, 3), (4, 8, 3)]                            # (B, D, n); n = B - 1: the band is the whole batch


def _tiny_row(case):
    case["u"][1] *= 1e-10 / float(case["u"][1].norm())       # norms far under eps = 1e-8
    case["v"][2] *= 1e-10 / float(case["v"][2].norm())
    return case


def _cases():
    cases = [inbatch64.make_case(3, B, D, n, True) for B, D, n in LITERAL]
    cases.append(inbatch64.make_case(4, 7, 5, 3, False))
    cases.append(_tiny_row(inbatch64.make_case(5, 7, 5, 3, True)))
    return cases


def test_restatement_equals_the_references_literal_expression():
    for case in _cases():
        want, got = inbatch64.literal(case), inbatch64.reference(case)["scores"]
        assert tuple(got.shape) == tuple(want.shape) == (case["dims"][0], case["n_neg"] + 1)
        assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), case["dims"]


def test_a_clamped_norm_is_a_constant_denominator():
    case = _tiny_row(inbatch64.make_case(5, 7, 5, 3, True))
    ref = inbatch64.reference(case)
    # d/du_1 of sum_k g_1k <u_1, v_j> / (eps max(|v_j|, eps)) / T: linear in u_1, no projection term
    B, n, T = 7, 3, case["temperature"]
    v, g = case["v"].double(), case["g"].double()
    want = sum(g[1, k] * v[(1 + k) % B] / (inbatch64.EPS * max(float(v[(1 + k) % B].norm()), inbatch64.EPS)) for k in range(n + 1)) / T
    assert float((ref["du"][1] - want).abs().max()) <= 1e-9 * float(want.abs().max())
    for name in inbatch64.names(case):
        assert bool(torch.isfinite(ref[name]).all()), name


def test_composition_equals_the_restatement():
    from recbox_amd import ops
    for case in _cases() + [inbatch64.make_case(6, 33, 20, 17, True), inbatch64.make_case(7, 2, 4, 1, True)]:
        want, ref32 = inbatch64.reference(case), inbatch64.reference(case, torch.float32)
        for tag, fn in (("torch", ops.inbatch_band_scores_torch), ("op on cpu", ops.inbatch_band_scores)):
            got = inbatch64.run(fn, case, "cpu")
            for name in inbatch64.names(case):
                fp32_bar.assert_bar("%s %s %s" % (name, tag, case["dims"]), got[name], want[name], ref32[name])
        c64 = dict(case, u=case["u"].double(), v=case["v"].double(), w=None if case["w"] is None else case["w"].double())
        got = inbatch64.run(ops.inbatch_band_scores_torch, c64, "cpu")
        for name in inbatch64.names(case):
            assert float((got[name] - want[name]).abs().max()) <= 1e-12 * max(1.0, float(want[name].abs().max())), name


def test_composition_never_forms_the_square(monkeypatch):
    """Every tensor the composition's forward creates stays under B (n_neg + 1) D elements."""
    from recbox_amd import ops
    case = inbatch64.make_case(3, 64, 8, 2, True)
    seen = []

    class Watch(torch.utils._python_dispatch.TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            out = func(*args, **(kwargs or {}))
            if isinstance(out, torch.Tensor):
                seen.append(out.numel())
            return out

    with Watch():
        ops.inbatch_band_scores_torch(case["u"], case["v"], 2, weight=case["w"])
    assert seen and max(seen) <= 64 * 3 * 8 < 64 * 64


def _check_step(which, tag, device, model=None, fx=None, tol=1e-5):
    if model is None:
        model, fx = inbatch64.loaded(which, device)
    outs, grads = inbatch64.step(which, model, fx, tag, device)
    for k, t in outs.items():
        err = inbatch64.rel_err(t, fx["out_%s_%s" % (which, tag)][k])
        assert err <= tol, "%s %s %s: %.3e" % (which, tag, k, err)
    for name, grad in grads.items():
        recorded = fx["g_%s_%s" % (which, tag)]
        err = inbatch64.rel_err(grad, recorded[name], inbatch64.grad_scale(model, name, recorded))
        assert err <= tol, "%s %s grad %s: %.3e" % (which, tag, name, err)
    return model, fx


@pytest.mark.parametrize("which,tag", [("sbc", "full"), ("sbc", "short"), ("fb", "full")])
def test_mirror_matches_the_reference_on_the_cpu_route(which, tag):
    model, fx = _check_step(which, tag, "cpu")
    assert list(model.state_dict().keys()) == [str(k) for k in fx["keys"][which]]


def test_short_batch_then_full_batch_gives_the_full_batchs_values():
    model, fx = _check_step("sbc", "short", "cpu")
    index1 = model.index1.copy()
    _check_step("sbc", "full", "cpu", model, fx)
    assert np.array_equal(model.index1, index1)


def test_a_short_batch_inside_the_band_goes_through_the_op(monkeypatch):
    """b + n_neg <= batch_size: the reference's double fold is (i + k) mod b, which the band op serves."""
    import gen_golden_inbatch as gen
    from recbox_amd import ops
    from recbox_amd.rechub.basic import features
    from recbox_amd.rechub.models import matching
    user = [features.SparseFeature("u0", vocab_size=11, embed_dim=4)]
    item = [features.SparseFeature("i0", vocab_size=13, embed_dim=4)]
    tower = {"dims": [8], "activation": "relu", "dropout": 0.0}
    model = matching.YoutubeSBC(user, item, [features.DenseFeature("sw")], dict(tower), dict(tower), batch_size=12, n_neg=3)
    calls = []
    real = ops.inbatch_band_scores
    monkeypatch.setattr(ops, "inbatch_band_scores", lambda *a, **k: calls.append(a[0].shape[0]) or real(*a, **k))
    g = torch.Generator().manual_seed(1)
    for rows in (12, 9, 10):
        x = {"u0": torch.randint(0, 11, (rows,), generator=g), "i0": torch.randint(0, 13, (rows,), generator=g),
             "sw": 0.05 + 0.95 * torch.rand(rows, generator=g)}
        got = model(x)
        index1 = model.index1[:rows * 4].copy()
        index1[np.where(index1 >= rows)] -= rows
        u, v = model.user_tower(x), model.item_tower(x)
        want = (torch.cosine_similarity(u.unsqueeze(1), v, dim=2) - torch.log(x["sw"]))[model.index0[:rows * 4], index1].view(-1, 4)
        assert float((got - want).detach().abs().max()) <= 1e-5, rows
    assert calls == [12, 9] and gen.N_NEG == 3


@pytest.mark.parametrize("which", ["sbc", "fb"])
def test_modes_return_the_tower_outputs(which):
    for mode in ("user", "item"):
        model, fx = inbatch64.loaded(which, "cpu")
        model.mode = mode
        got = model(fx.tensors("in_%s_full" % which))
        assert inbatch64.rel_err(got, fx["mode_" + which][mode]) <= 1e-5, (which, mode)


def test_committed_seeds_keep_every_relu_input_away_from_zero():
    import gen_golden_inbatch as gen
    fx = Fixture("rechub_inbatch")
    for which in ("sbc", "fb"):
        assert float(fx["seed"][which][1]) > gen.MIN_PRE_RELU, which


def test_losses_match_the_reference():
    from recbox_amd.rechub.basic.loss_func import BPRLoss, HingeLoss
    fx = Fixture("rechub_inbatch")
    t = fx.tensors("loss")
    assert inbatch64.rel_err(HingeLoss()(t["pos"], t["neg"]), fx["loss"]["hinge"]) <= 1e-6
    assert inbatch64.rel_err(BPRLoss()(t["pos"], t["neg"][:, 0]), fx["loss"]["bpr_pairs"]) <= 1e-6
    assert inbatch64.rel_err(BPRLoss()(t["pos"].view(-1, 1), t["neg"]), fx["loss"]["bpr_rows"]) <= 1e-6
    # num_items: the share of negatives inside the margin, as a float
    pos, neg = t["pos"].double(), t["neg"].double()
    base = torch.clamp(neg.max(1).values - pos + 2, min=0)
    rank = ((neg - pos.view(-1, 1) + 2) > 0).double().mean(1) * 50
    got = HingeLoss(num_items=50)(t["pos"], t["neg"])
    assert abs(float(got) - float((base * torch.log(rank + 1)).mean())) <= 1e-5


def test_n_neg_at_or_above_the_batch_raises():
    from recbox_amd import ops
    case = inbatch64.make_case(3, 4, 8, 3, True)
    for fn in (ops.inbatch_band_scores, ops.inbatch_band_scores_torch):
        for n in (4, 5):
            with pytest.raises(ValueError):
                fn(case["u"], case["v"], n, weight=case["w"])
        assert tuple(fn(case["u"], case["v"], 3, weight=case["w"]).shape) == (4, 4)


def test_compat_paths_resolve_to_the_mirrors():
    from recbox_amd import compat
    from recbox_amd.rechub.basic import loss_func
    from recbox_amd.rechub.models import matching
    table, also = compat.alias_table(), compat.alias_also()
    for root in ("torch_rechub", "recbox.third_party.rechub"):
        assert table[root + ".models.matching.youtube_sbc"] == ("recbox_amd.rechub.models.matching", ["YoutubeSBC"])
        assert table[root + ".models.matching.dssm_facebook"] == ("recbox_amd.rechub.models.matching", ["FaceBookDSSM"])
        assert table[root + ".basic.loss_func"] == ("recbox_amd.rechub.basic.loss_func", ["HingeLoss", "BPRLoss"])
        names = table[root + ".models.matching"][1] + also.get(root + ".models.matching", [])
        assert "YoutubeSBC" in names and "FaceBookDSSM" in names
    report = compat.install(prefixes=("torch_rechub", "recbox"), overlay=False)
    try:
        for root in ("torch_rechub", "recbox.third_party.rechub"):
            for path, name, target in ((".models.matching", "YoutubeSBC", matching), (".models.matching", "FaceBookDSSM", matching),
                                       (".models.matching.youtube_sbc", "YoutubeSBC", matching),
                                       (".models.matching.dssm_facebook", "FaceBookDSSM", matching),
                                       (".basic.loss_func", "HingeLoss", loss_func), (".basic.loss_func", "BPRLoss", loss_func)):
                mod = importlib.import_module(root + path)
                assert hasattr(mod, name), (root, path, name)
                if getattr(mod, "__recbox_amd__", False):
                    assert getattr(mod, name) is getattr(target, name)
    finally:
        compat.uninstall(report)


def test_header_declares_the_entry_points():
    with open(os.path.join(ROOT, "include", "recbox_hip.h")) as fh:
        text = fh.read()
    for name in NAMES + OTHER:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name


def test_library_exports_and_lib_binds_them():
    from recbox_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES + OTHER:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES
        assert getattr(_lib.lib, name).argtypes == _lib.SIGNATURES[name][1]


def test_supported_answers_without_a_device():
    from recbox_amd import _lib, ops
    lib = _lib.lib
    assert [ops.inbatch_band_max_neg(D) for D in (4, 64, 128, 256, 512)] == [64, 64, 64, 50, 22]
    assert [ops.inbatch_band_max_neg(D) for D in (0, 6, 516, -4)] == [0, 0, 0, 0]
    for D in (4, 20, 64, 100, 256, 512):
        cap = ops.inbatch_band_max_neg(D)
        assert (16 + cap) * (2 * D + 2 * cap + 4) * 4 <= 160 * 1024
        assert cap == 64 or (16 + cap + 1) * (2 * D + 2 * (cap + 1) + 4) * 4 > 160 * 1024
        assert lib.rbx_inbatch_band_supported(D, cap, _lib.RBX_F32) == 1 and lib.rbx_inbatch_band_supported(D, cap + 1, _lib.RBX_F32) == 0
        assert ops.inbatch_band_supported(cap + 1, D, cap) and not ops.inbatch_band_supported(cap, D, cap)
    assert lib.rbx_inbatch_band_supported(64, 0, _lib.RBX_F32) == 0 and lib.rbx_inbatch_band_supported(64, 3, _lib.RBX_F64) == 0
    assert not ops.inbatch_band_supported(64, 6, 3) and not ops.inbatch_band_supported(64, 516, 3)
    assert not ops.inbatch_band_supported(64, 64, 3, torch.float64) and not ops.inbatch_band_supported(64, 64, 3, torch.float16)


def test_refusals_come_before_any_launch():
    from recbox_amd import _lib
    lib, p = _lib.lib, 0x1000                               # fake, never dereferenced: every refusal precedes the launch

    def fwd(D, n, batch=128, dtype=_lib.RBX_F32, us=None, ss=None, base=p):
        return lib.rbx_inbatch_band_fwd(base, D if us is None else us, p, D, p, batch, D, n, 1e-8, 1.0, dtype, p,
                                        n + 1 if ss is None else ss, p, p, None)

    def bwd(D, n, batch=128, dtype=_lib.RBX_F32, us=None, ss=None, base=p):
        return lib.rbx_inbatch_band_bwd(p, n + 1 if ss is None else ss, base, D if us is None else us, p, D, p, p, p, batch, D, n,
                                        1e-8, 1.0, dtype, p, D, p, D, p, None)

    for call in (fwd, bwd):
        for D, n, batch in ((6, 3, 128), (516, 3, 128), (64, 65, 128), (512, 23, 128), (64, 0, 128), (64, 8, 8), (64, 9, 8)):
            assert call(D, n, batch) == _lib.RBX_ERR_UNSUPPORTED, (call.__name__, D, n, batch)
            assert _lib.last_error()
        assert call(64, 3, dtype=_lib.RBX_F64) == _lib.RBX_ERR_UNSUPPORTED
        assert call(64, 3, batch=-1) == _lib.RBX_ERR_INVALID
        assert call(64, 3, us=60) == _lib.RBX_ERR_INVALID                       # a row stride shorter than the row
        assert call(64, 3, us=66) == _lib.RBX_ERR_INVALID                       # rows that are not 16-byte aligned
        assert call(64, 3, base=p + 4) == _lib.RBX_ERR_INVALID
        assert call(64, 3, ss=3) == _lib.RBX_ERR_INVALID
        assert call(64, 3, batch=0) == _lib.RBX_OK                              # empty batch: nothing launched


def test_op_falls_back_without_raising(monkeypatch):
    from recbox_amd import ops
    case = inbatch64.make_case(3, 6, 8, 3, True)
    out = ops.inbatch_band_scores(case["u"], case["v"], 3, weight=case["w"], temperature=0.5)
    assert torch.equal(out, ops.inbatch_band_scores_torch(case["u"], case["v"], 3, weight=case["w"], temperature=0.5))
    assert tuple(ops.inbatch_band_scores(case["u"][:0], case["v"][:0], 3).shape) == (0, 4)
    assert ops.inbatch_band_scores(case["u"].double(), case["v"].double(), 3).dtype == torch.float64
    monkeypatch.setattr(ops.config, "inbatch_fused", False)
    assert torch.equal(ops.inbatch_band_scores(case["u"], case["v"], 3, weight=case["w"], temperature=0.5), out)


def test_switch_is_spelled_like_its_neighbours():
    from recbox_amd import ops
    assert ops.config.inbatch_fused is True or os.environ.get("RECBOX_AMD_INBATCH_FUSED") == "0"
    with open(os.path.join(ROOT, "recbox_amd", "ops.py")) as fh:
        assert 'inbatch_fused = os.environ.get("RECBOX_AMD_INBATCH_FUSED", "1") != "0"' in fh.read()
