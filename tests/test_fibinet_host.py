"""FiBiNet's ops (``ops.senet_gate`` / ``ops.bilinear_pairs``, csrc/rbx_bilinear.hip) and mirrors, the parts that need no GPU:
the compositions against the float64 restatement of tests/fibinet64.py under the fp32-scaled bar; the restatement's hand-written
backward against autograd in float64; the seeds of the cases; SENETLayer, BiLinearInteractionLayer and FiBiNet on the CPU against
the live reference's fixture (tests/golden/rechub_fibinet.npz, written by tests/gen_golden_fibinet.py) with its ordered
state_dict keys; the compat paths; the C ABI's entries and their refusals; the fall-backs of the ops."""
import ctypes
import importlib
import os
import re

import pytest
import torch

import fibinet64
import fp32_bar
import test_gpu_fibinet_forms as forms
from conftest import Fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["rbx_senet_gate_supported", "rbx_senet_gate_fwd", "rbx_senet_gate_bwd_workspace_size", "rbx_senet_gate_bwd",
         "rbx_bilinear_pairs_supported", "rbx_bilinear_pairs_fwd", "rbx_bilinear_pairs_bwd_workspace_size",
         "rbx_bilinear_pairs_bwd"]
SHAPES = [(1, 2, 4), (7, 3, 8), (9, 5, 16), (5, 26, 8), (6, 7, 6)]


@pytest.mark.parametrize("with_scale", [True, False])
@pytest.mark.parametrize("act", ["relu", "sigmoid"])
@pytest.mark.parametrize("kind", fibinet64.KINDS)
def test_compositions_equal_the_float64_restatement(kind, act, with_scale):
    from recbox_amd import ops
    for n, (B, F, D) in enumerate(SHAPES):
        case = fibinet64.make_case(3, B, F, D, kind, act=act, transposed=bool(n & 1))
        want, ref32 = fibinet64.reference(case, with_scale), fibinet64.reference(case, with_scale, torch.float32)
        for tag, fns in (("torch", (ops.senet_gate_torch, ops.bilinear_pairs_torch)), ("op on cpu", (ops.senet_gate, ops.bilinear_pairs))):
            got = fibinet64.run(fns[0], fns[1], case, "cpu", with_scale)
            for name in fibinet64.NAMES:
                fp32_bar.assert_bar("%s %s %s" % (name, tag, (B, F, D)), got[name], want[name], ref32[name])


@pytest.mark.parametrize("kind", fibinet64.KINDS)
def test_restatement_backward_equals_autograd_in_float64(kind):
    from recbox_amd import ops
    for tr, act, ws in ((False, "relu", True), (True, "sigmoid", True), (True, "relu", False)):
        case = fibinet64.make_case(9, 5, 4, 8, kind, act=act, transposed=tr)
        want = fibinet64.reference(case, ws)
        c64 = dict(case, **{k: case[k].double() for k in ("x", "w1", "w2", "W", "up", "upa")})
        got = fibinet64.run(ops.senet_gate_torch, ops.bilinear_pairs_torch, c64, "cpu", ws)
        for name in fibinet64.NAMES:
            assert float((got[name] - want[name]).abs().max()) <= 1e-12 * max(1.0, float(want[name].abs().max())), name


def test_seeds_stay_away_from_the_kinks_and_the_gate_opens_and_closes():
    for F in (2, 3, 5, 26):
        closed = opened = False
        for kind in fibinet64.KINDS:
            case = fibinet64.make_case(11, 17, F, 8, kind)
            assert fibinet64.kink_margin(case["x"], case["w1"], case["w2"], "relu") > fibinet64.KINK
            a = fibinet64.gate64(case["x"], case["w1"], case["w2"], "relu")[0]
            closed, opened = closed or bool((a == 0).any()), opened or bool((a > 0).any())
        assert closed and opened, F


def test_the_form_cases_cover_every_form_of_the_launch_geometry():
    forms.check_the_list_covers_every_form()


@pytest.mark.parametrize("name", list(forms.CASES))
def test_a_form_case_reaches_its_form_and_its_references_hold_the_bar(name):
    """What tests/test_gpu_fibinet_forms.py sends to the GPU, judged here first: the case selects the launch geometry its table
    names (the chunk count and the gate's grid read from the library), its seed keeps every ReLU of the gate KINK away from
    zero, the fp32 restatement is finite and under the bar, and another fp32 summation order -- the composition on the CPU --
    holds the same bar against float64."""
    from recbox_amd import ops
    forms.check_forms(name)
    case, (want, ref32) = forms._case(name)
    ws = forms.CASES[name][0][6]
    assert fibinet64.kink_margin(case["x"], case["w1"], case["w2"], case["act"]) >= fibinet64.KINK
    got = fibinet64.run(ops.senet_gate_torch, ops.bilinear_pairs_torch, case, "cpu", ws)
    for key in fibinet64.NAMES:
        assert bool(torch.isfinite(ref32[key]).all()), key
        fp32_bar.assert_bar("%s ref32 %s" % (key, name), ref32[key], want[key], ref32[key])
        fp32_bar.assert_bar("%s composition %s" % (key, name), got[key], want[key], ref32[key])


@pytest.mark.parametrize("kind", fibinet64.KINDS)
def test_model_matches_the_reference_on_the_cpu_path(kind):
    model, _ = fibinet64.check_model_against_fixture(kind, "cpu")
    fx = Fixture("rechub_fibinet")
    assert list(model.state_dict().keys()) == [str(k) for k in fx["keys"][kind]]
    assert model.dims == 5 * 4 * 8 and tuple(model.senet_layer.mlp[0].weight.shape) == (1, 5)


def test_layers_alone_match_the_reference():
    from recbox_amd.rechub.basic.layers import BiLinearInteractionLayer, SENETLayer
    fx = Fixture("rechub_fibinet")
    x = torch.from_numpy(fx["layer"]["x"])
    senet = SENETLayer(5, 3)
    assert list(senet.state_dict().keys()) == ["mlp.0.weight", "mlp.2.weight"]
    senet.load_state_dict({k: torch.from_numpy(v) for k, v in fx["senet"].items() if k != "out"}, strict=True)
    assert fibinet64.rel_err(senet(x), fx["senet"]["out"]) <= 1e-5
    for kind in fibinet64.KINDS:
        layer = BiLinearInteractionLayer(8, 5, kind)
        assert list(layer.state_dict().keys()) == [str(k) for k in fx["keys_bi"][kind]]
        layer.load_state_dict({k: torch.from_numpy(v) for k, v in fx["bi_" + kind].items() if k != "out"}, strict=True)
        out = layer(x)
        assert tuple(out.shape) == (6, 10, 8) and fibinet64.rel_err(out, fx["bi_" + kind]["out"]) <= 1e-5
    assert list(BiLinearInteractionLayer(8, 5, "field_all").state_dict().keys()) == ["bilinear_layer.weight"]
    assert "bilinear_layer.9.weight" in BiLinearInteractionLayer(8, 5).state_dict()
    with pytest.raises(NotImplementedError):
        BiLinearInteractionLayer(8, 5, "field_some")


def test_compat_paths_resolve_to_the_mirrors():
    from recbox_amd import compat
    from recbox_amd.rechub.basic import layers
    from recbox_amd.rechub.models import ranking
    table, also = compat.alias_table(), compat.alias_also()
    for root in ("torch_rechub", "recbox.third_party.rechub"):
        assert table[root + ".models.ranking.fibinet"] == ("recbox_amd.rechub.models.ranking", ["FiBiNet"])
        assert "FiBiNet" in also[root + ".models.ranking"]
    report = compat.install(prefixes=("torch_rechub", "recbox"), overlay=False)
    try:
        for root in ("torch_rechub", "recbox.third_party.rechub"):
            for path, name, target in ((".models.ranking", "FiBiNet", ranking), (".models.ranking.fibinet", "FiBiNet", ranking),
                                       (".basic.layers", "SENETLayer", layers), (".basic.layers", "BiLinearInteractionLayer", layers)):
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


def test_supported_answers_without_a_launch():
    from recbox_amd import _lib, ops
    lib = _lib.lib
    for F, D in ((2, 4), (64, 32), (26, 16), (39, 8)):
        assert lib.rbx_bilinear_pairs_supported(F, D, _lib.RBX_F32) == 1 and lib.rbx_senet_gate_supported(F, D, max(1, F // 3), _lib.RBX_F32) == 1
        assert ops.bilinear_pairs_supported(F, D) and ops.senet_gate_supported(F, D, max(1, F // 3))
    for F, D, dt in ((5, 6, _lib.RBX_F32), (5, 0, _lib.RBX_F32), (1, 8, _lib.RBX_F32), (65, 8, _lib.RBX_F32), (5, 8, _lib.RBX_F64)):
        assert lib.rbx_bilinear_pairs_supported(F, D, dt) == 0, (F, D, dt)
        assert lib.rbx_senet_gate_supported(F, D, 1, dt) == 0, (F, D, dt)
    assert lib.rbx_senet_gate_supported(5, 8, 0, _lib.RBX_F32) == 0
    assert not ops.bilinear_pairs_supported(5, 8, torch.float64) and not ops.bilinear_pairs_supported(5, 8, torch.float16)
    assert not ops.senet_gate_supported(5, 64, 1) and not ops.bilinear_pairs_supported(5, 64)


def test_refusals_come_before_any_launch():
    from recbox_amd import _lib
    lib, p = _lib.lib, 0x1000                               # fake, never dereferenced: every refusal precedes the launch

    def fwd(F, D, dtype=_lib.RBX_F32, batch=4, x=p, xsb=None):
        return lib.rbx_bilinear_pairs_fwd(x, F * D if xsb is None else xsb, D, p, None, batch, F, D, 2, 0, dtype, p, F * (F - 1) // 2 * D, None)

    def bwd(F, D, dtype=_lib.RBX_F32, batch=4, x=p, xsb=None):
        return lib.rbx_bilinear_pairs_bwd(p, F * (F - 1) // 2 * D, x, F * D if xsb is None else xsb, D, p, None, batch, F, D, 2, 0,
                                          dtype, p, None, p, p, 1 << 40, None)

    def gfwd(F, D, dtype=_lib.RBX_F32, batch=4, x=p, xsb=None):
        return lib.rbx_senet_gate_fwd(x, F * D if xsb is None else xsb, D, p, p, batch, F, D, 1, 0, dtype, p, p, None)

    def gbwd(F, D, dtype=_lib.RBX_F32, batch=4, x=p, xsb=None):
        return lib.rbx_senet_gate_bwd(p, x, F * D if xsb is None else xsb, D, p, p, p, p, batch, F, D, 1, 0, dtype, 0, p, p, p, p, 1 << 40,
                                      None)

    for call in (fwd, bwd, gfwd, gbwd):
        for F, D in ((5, 6), (5, 0), (1, 8), (65, 8)):
            assert call(F, D) == _lib.RBX_ERR_UNSUPPORTED, (call.__name__, F, D)
            assert _lib.last_error()
        assert call(5, 8, dtype=_lib.RBX_F64) == _lib.RBX_ERR_UNSUPPORTED
        assert call(5, 8, x=p + 4) == _lib.RBX_ERR_UNSUPPORTED                  # a misaligned base
        assert call(5, 8, xsb=42) == _lib.RBX_ERR_UNSUPPORTED                   # a stride that is no multiple of 4
        assert call(5, 8, batch=-1) == _lib.RBX_ERR_INVALID
        assert call(5, 8, batch=0) == _lib.RBX_OK                               # empty batch: nothing launched
    assert lib.rbx_bilinear_pairs_bwd_workspace_size(0, 5, 8) == 0 and lib.rbx_bilinear_pairs_bwd_workspace_size(64, 5, 8) > 0
    assert lib.rbx_bilinear_pairs_bwd(p, 80, p, 40, 8, p, None, 4, 5, 8, 2, 0, _lib.RBX_F32, p, None, p, p, 16, None) \
        == _lib.RBX_ERR_WORKSPACE


def test_ops_fall_back_without_raising(monkeypatch):
    from recbox_amd import ops
    case = fibinet64.make_case(3, 6, 5, 8, "field_interaction")
    x, w1, w2, W = case["x"], case["w1"], case["w2"], case["W"]
    a = ops.senet_gate(x, w1, w2)
    assert torch.equal(a, ops.senet_gate_torch(x, w1, w2)) and tuple(a.shape) == (6, 5)
    out = ops.bilinear_pairs(x, W, "field_interaction", scale=a)
    assert torch.equal(out, ops.bilinear_pairs_torch(x, W, "field_interaction", False, a)) and tuple(out.shape) == (6, 20, 8)
    assert tuple(ops.bilinear_pairs(x, W, "field_interaction").shape) == (6, 10, 8)
    out64 = ops.bilinear_pairs(x.double(), W.double(), "field_interaction", scale=ops.senet_gate(x.double(), w1.double(), w2.double()))
    assert out64.dtype == torch.float64 and tuple(out64.shape) == (6, 20, 8)
    empty = ops.bilinear_pairs(x[:0], W, "field_interaction", scale=ops.senet_gate(x[:0], w1, w2))
    assert tuple(empty.shape) == (0, 20, 8)
    monkeypatch.setattr(ops.config, "bilinear_fused", False)
    assert torch.equal(ops.bilinear_pairs(x, W, "field_interaction", scale=a), out)
    with pytest.raises(NotImplementedError):
        ops.bilinear_pairs(x, W, "field_some")
    with pytest.raises(ValueError):
        ops.senet_gate(x, w1, w2, act="tanh")


def test_switch_is_spelled_like_its_neighbours():
    from recbox_amd import ops
    assert ops.config.bilinear_fused is True or os.environ.get("RECBOX_AMD_BILINEAR_FUSED") == "0"
    with open(os.path.join(ROOT, "recbox_amd", "ops.py")) as fh:
        assert 'bilinear_fused = os.environ.get("RECBOX_AMD_BILINEAR_FUSED", "1") != "0"' in fh.read()
