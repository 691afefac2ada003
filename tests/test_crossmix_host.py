"""DCN-V2's cross expert mixture (``ops.cross_mix``, csrc/rbx_crossmix.hip) and the Deep & Cross mirrors, the parts that need no
GPU: the composition against the float64 restatement of tests/crossmix64.py under the fp32-scaled bar; the seeds of the cases;
DCN, DCNv2, EDCN and WideDeep on the CPU against the live reference's fixture (tests/golden/rechub_dcn.npz, written by
tests/gen_golden_crossmix.py) with its ordered state_dict keys; the compat paths; the C ABI's entries and their refusals; the
fall-backs of the op."""
import ctypes
import importlib
import os
import re

import pytest
import torch

import crossmix64
import fp32_bar
import test_gpu_crossmix_forms as forms
from conftest import Fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["rbx_crossmix_supported", "rbx_crossmix_fwd", "rbx_crossmix_bwd_workspace_size", "rbx_crossmix_bwd"]
SHAPES = [(1, 3, 1, 4, 1), (7, 17, 3, 8, 2), (9, 40, 4, 32, 3), (5, 16, 2, 6, 2), (6, 130, 4, 64, 1)]       # (B, n, E, r, L)


def test_composition_equals_the_float64_restatement():
    from recbox_amd import ops
    for B, n, E, r, L in SHAPES:
        case = crossmix64.make_case(3, B, n, E, r, L)
        want, ref32 = crossmix64.reference(case), crossmix64.reference(case, torch.float32)
        for tag, fn in (("torch", ops.cross_mix_torch), ("op on cpu", ops.cross_mix)):
            got = crossmix64.run(fn, case, "cpu")
            for name in crossmix64.names(L):
                fp32_bar.assert_bar("%s %s %s" % (name, tag, (B, n, E, r, L)), got[name], want[name], ref32[name])


def test_composition_in_float64_equals_the_restatement():
    from recbox_amd import ops
    case = crossmix64.make_case(5, 6, 17, 3, 8, 2)
    want = crossmix64.reference(case)
    c64 = dict(case, x0=case["x0"].double(), G=case["G"].double(), up=case["up"].double(),
               **{k: [t.double() for t in case[k]] for k in ("U", "V", "C", "b")})
    got = crossmix64.run(ops.cross_mix_torch, c64, "cpu")
    for name in crossmix64.names(2):
        assert float((got[name] - want[name]).abs().max()) <= 1e-12 * max(1.0, float(want[name].abs().max())), name


def test_seeds_reach_the_saturated_branch_of_tanh_and_mostly_stay_out_of_it():
    for B, n, E, r, L in ((33, 40, 4, 32, 3), (257, 416, 4, 32, 1), (17, 17, 3, 8, 1)):
        a = crossmix64.tanh_inputs(crossmix64.make_case(11, B, n, E, r, L)).abs()
        frac = float((a > 3).double().mean())
        assert 0.0 < frac < 0.5, (B, n, E, r, L, frac)


def test_the_form_cases_cover_every_form_of_the_launch_geometry():
    forms.check_the_list_covers_every_form()
    reached = 0
    for name in forms.CASES:
        a = crossmix64.tanh_inputs(forms.make(name)).abs()
        assert bool(torch.isfinite(a).all()) and float((a > 3).double().mean()) < 0.5, name
        reached += int((a > 3).sum())
    assert reached > 0


@pytest.mark.parametrize("name", list(forms.CASES))
def test_a_form_case_reaches_its_form_and_its_references_hold_the_bar(name):
    """What tests/test_gpu_crossmix_forms.py sends to the GPU, judged here first: the case selects the launch geometry its table
    names, the library takes it, the fp32 restatement is finite and under the bar, and another fp32 summation order -- the
    composition on the CPU -- holds the same bar against float64."""
    from recbox_amd import ops
    forms.check_forms(name)
    case, (want, ref32) = forms._case(name)
    got = crossmix64.run(ops.cross_mix_torch, case, "cpu")
    for key in crossmix64.names(forms.CASES[name][0][4]):
        assert bool(torch.isfinite(ref32[key]).all()), key
        fp32_bar.assert_bar("%s ref32 %s" % (key, name), ref32[key], want[key], ref32[key])
        fp32_bar.assert_bar("%s composition %s" % (key, name), got[key], want[key], ref32[key])


@pytest.mark.parametrize("which", crossmix64.MODELS)
def test_model_matches_the_reference_on_the_cpu_path(which):
    model, _ = crossmix64.check_model_against_fixture(which, "cpu")
    fx = Fixture("rechub_dcn")
    assert list(model.state_dict().keys()) == [str(k) for k in fx["keys"][which]]


def test_committed_seeds_keep_every_relu_input_away_from_zero():
    import gen_golden_crossmix as gen
    fx = Fixture("rechub_dcn")
    for which in crossmix64.MODELS:
        assert float(fx["seed"][which][1]) > gen.MIN_PRE_RELU, which


def test_mixture_parameter_names_and_edcn_overwrites_the_callers_dims():
    from recbox_amd.rechub.basic import features
    from recbox_amd.rechub.basic.layers import CrossLayer, CrossNetMix, CrossNetV2, CrossNetwork
    from recbox_amd.rechub.models.ranking import EDCN
    mix = CrossNetMix(12, num_layers=2, low_rank=4, num_experts=3)
    assert list(mix.state_dict().keys()) == ["u_list.0", "u_list.1", "v_list.0", "v_list.1", "c_list.0", "c_list.1",
                                             "gating.0.weight", "gating.1.weight", "gating.2.weight", "bias.0", "bias.1"]
    assert tuple(mix.u_list[0].shape) == (3, 12, 4) and tuple(mix.c_list[1].shape) == (3, 4, 4) and tuple(mix.bias[0].shape) == (12, 1)
    assert list(CrossNetwork(12, 2).state_dict().keys()) == ["w.0.weight", "w.1.weight", "b.0", "b.1"]
    assert tuple(CrossNetV2(12, 1).w[0].weight.shape) == (12, 12) and CrossNetV2(12, 1).w[0].bias is None
    assert list(CrossLayer(12).state_dict().keys()) == ["b", "w.weight"]
    feats = [features.SparseFeature("s%d" % i, vocab_size=5, embed_dim=4) for i in range(3)]
    params = {"dims": [7], "dropout": 0.0}
    EDCN(feats, 1, params)
    assert params["dims"] == [12, 12]


def test_a_batch_of_one_returns_a_vector_as_the_reference_does():
    from recbox_amd import ops
    from recbox_amd.rechub.basic.layers import CrossNetMix
    mix = CrossNetMix(12, num_layers=2, low_rank=4, num_experts=3)
    assert tuple(mix(torch.randn(1, 12)).shape) == (12,) and tuple(mix(torch.randn(5, 12)).shape) == (5, 12)
    case = crossmix64.make_case(3, 1, 12, 3, 4, 2)
    assert tuple(ops.cross_mix(case["x0"], case["U"], case["V"], case["C"], case["G"], case["b"]).shape) == (1, 12)


def test_compat_paths_resolve_to_the_mirrors():
    from recbox_amd import compat
    from recbox_amd.rechub.basic import layers
    from recbox_amd.rechub.models import ranking
    table, also = compat.alias_table(), compat.alias_also()
    for root in ("torch_rechub", "recbox.third_party.rechub"):
        assert table[root + ".models.ranking.dcn_v2"] == ("recbox_amd.rechub.models.ranking", ["DCNv2"])
        for name in ("DCN", "DCNv2", "EDCN", "WideDeep"):
            assert name in also[root + ".models.ranking"]
    report = compat.install(prefixes=("torch_rechub", "recbox"), overlay=False)
    try:
        for root in ("torch_rechub", "recbox.third_party.rechub"):
            for path, name, target in ((".models.ranking", "DCNv2", ranking), (".models.ranking", "DCN", ranking),
                                       (".models.ranking", "EDCN", ranking), (".models.ranking", "WideDeep", ranking),
                                       (".models.ranking.dcn", "DCN", ranking), (".models.ranking.dcn_v2", "DCNv2", ranking),
                                       (".models.ranking.edcn", "EDCN", ranking), (".models.ranking.edcn", "BridgeModule", ranking),
                                       (".models.ranking.widedeep", "WideDeep", ranking), (".basic.layers", "CrossNetMix", layers),
                                       (".basic.layers", "CrossNetV2", layers), (".basic.layers", "CrossNetwork", layers),
                                       (".basic.layers", "CrossLayer", layers)):
                mod = importlib.import_module(root + path)
                assert hasattr(mod, name), (root, path, name)
                if getattr(mod, "__recbox_amd__", False):
                    assert getattr(mod, name) is getattr(target, name)
    finally:
        compat.uninstall(report)


def test_header_declares_the_entry_points():
    with open(os.path.join(ROOT, "include", "recbox_hip.h")) as fh:
        text = fh.read()
    for name in NAMES:
        assert re.search(r"\b(int|size_t)\s+%s\s*\(" % name, text), name


def test_library_exports_and_lib_binds_them():
    from recbox_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES
        assert getattr(_lib.lib, name).argtypes == _lib.SIGNATURES[name][1]


def test_supported_answers_without_a_device():
    from recbox_amd import _lib, ops
    lib = _lib.lib
    for n, E, r in ((416, 4, 32), (624, 4, 8), (1, 1, 4), (640, 4, 64), (3, 8, 32), (40, 2, 16)):
        assert lib.rbx_crossmix_supported(n, E, r, _lib.RBX_F32) == 1 and ops.cross_mix_supported(n, E, r), (n, E, r)
    for n, E, r, dt in ((40, 2, 6, _lib.RBX_F32), (40, 8, 64, _lib.RBX_F32), (40, 5, 64, _lib.RBX_F32), (641, 4, 32, _lib.RBX_F32),
                        (0, 4, 32, _lib.RBX_F32), (40, 0, 32, _lib.RBX_F32), (40, 9, 4, _lib.RBX_F32), (40, 2, 128, _lib.RBX_F32),
                        (40, 4, 32, _lib.RBX_F64)):
        assert lib.rbx_crossmix_supported(n, E, r, dt) == 0, (n, E, r, dt)
    assert not ops.cross_mix_supported(40, 2, 6) and not ops.cross_mix_supported(40, 8, 64) and not ops.cross_mix_supported(641, 4, 32)
    assert not ops.cross_mix_supported(40, 4, 32, torch.float64) and not ops.cross_mix_supported(40, 4, 32, torch.float16)


def test_refusals_come_before_any_launch():
    from recbox_amd import _lib
    lib, p = _lib.lib, 0x1000                               # fake, never dereferenced: every refusal precedes the launch

    def fwd(n, E, r, dtype=_lib.RBX_F32, batch=4, xs=None, os_=None):
        return lib.rbx_crossmix_fwd(p, n if xs is None else xs, p, n, p, p, p, p, p, batch, n, E, r, dtype, p,
                                    n if os_ is None else os_, None)

    def bwd(n, E, r, dtype=_lib.RBX_F32, batch=4, xs=None, os_=None, ws=1 << 40):
        return lib.rbx_crossmix_bwd(p, n if os_ is None else os_, p, n if xs is None else xs, p, n, p, p, p, p, p, batch, n, E, r,
                                    dtype, 0, p, n, p, n, p, p, p, p, p, p, ws, None)

    for call in (fwd, bwd):
        for n, E, r in ((40, 2, 6), (40, 8, 64), (641, 4, 32), (40, 9, 4)):
            assert call(n, E, r) == _lib.RBX_ERR_UNSUPPORTED, (call.__name__, n, E, r)
            assert _lib.last_error()
        assert call(40, 4, 32, dtype=_lib.RBX_F64) == _lib.RBX_ERR_UNSUPPORTED
        assert call(40, 4, 32, batch=-1) == _lib.RBX_ERR_INVALID
        assert call(40, 4, 32, xs=39) == _lib.RBX_ERR_INVALID                   # a row stride shorter than the row
        assert call(40, 4, 32, os_=39) == _lib.RBX_ERR_INVALID
        assert call(40, 4, 32, batch=0) == _lib.RBX_OK                          # empty batch: nothing launched
    assert lib.rbx_crossmix_bwd_workspace_size(0, 40, 4, 32) == 0 and lib.rbx_crossmix_bwd_workspace_size(64, 40, 4, 32) > 0
    assert lib.rbx_crossmix_bwd_workspace_size(64, 40, 2, 6) == 0
    assert bwd(40, 4, 32, ws=16) == _lib.RBX_ERR_WORKSPACE


def test_op_falls_back_without_raising(monkeypatch):
    from recbox_amd import ops
    case = crossmix64.make_case(3, 6, 17, 3, 8, 2)
    args = (case["U"], case["V"], case["C"], case["G"], case["b"])
    out = ops.cross_mix(case["x0"], *args)
    assert torch.equal(out, ops.cross_mix_torch(case["x0"], *args)) and tuple(out.shape) == (6, 17)
    assert tuple(ops.cross_mix(case["x0"][:0], *args).shape) == (0, 17)
    out64 = ops.cross_mix(case["x0"].double(), *[[t.double() for t in a] if isinstance(a, list) else a.double() for a in args])
    assert out64.dtype == torch.float64
    monkeypatch.setattr(ops.config, "crossmix_fused", False)
    assert torch.equal(ops.cross_mix(case["x0"], *args), out)


def test_switch_is_spelled_like_its_neighbours():
    from recbox_amd import ops
    assert ops.config.crossmix_fused is True or os.environ.get("RECBOX_AMD_CROSSMIX_FUSED") == "0"
    with open(os.path.join(ROOT, "recbox_amd", "ops.py")) as fh:
        assert 'crossmix_fused = os.environ.get("RECBOX_AMD_CROSSMIX_FUSED", "1") != "0"' in fh.read()
