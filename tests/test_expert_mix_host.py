"""Expert-gate mixing (``ops.expert_mix``, csrc/rbx_mix.hip) and the multi-task mirrors, the parts that need no GPU: the cat /
mul / sum composition against the float64 restatement of tests/mix64.py; the op on CPU tensors; SharedBottom, ESMM, MMOE, PLE
and AITM on the CPU path against the live reference's fixture (tests/golden/rechub_multi_task.npz, written by
tests/gen_golden_multi_task.py) with its ordered state_dict keys; the C ABI's entries and their refusals; the gate on the
edges of its range; the compat paths."""
import ctypes
import importlib
import os
import re

import pytest
import torch

import mix64
from conftest import Fixture, assert_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["rbx_expert_mix_supported", "rbx_expert_mix_fwd", "rbx_expert_mix_bwd"]
TAGS = ["shared_bottom", "esmm", "mmoe", "ple", "aitm"]
TOL = 1e-4

CASES = {
    "all": (5, 12, 3, mix64.full_select(3, 2)),
    "ple": (7, 8, 5, mix64.ple_select(2, 2, 1)),
    "unused_and_unordered": (4, 16, 4, [[2, 0], [0, 3, 2]]),                   # expert 1 unused, expert 0 and 2 in every gate
    "one": (3, 4, 1, [[0]]),
}


def _compare(got, want, what, grads=True):
    for t, (a, b) in enumerate(zip(got["out"], want["out"])):
        assert_close(a, b, TOL, "%s out %d" % (what, t))
    if grads:
        for e, (a, b) in enumerate(zip(got["dx"], want["dx"])):
            assert_close(a if a is not None else torch.zeros_like(b), b, TOL, "%s dx %d" % (what, e))
        for t, (a, b) in enumerate(zip(got["dz"], want["dz"])):
            assert_close(a if a is not None else torch.zeros_like(b), b, TOL, "%s dz %d" % (what, t))


@pytest.mark.parametrize("softmax", [True, False])
@pytest.mark.parametrize("name", sorted(CASES))
def test_composition_equals_the_float64_restatement(name, softmax):
    from recbox_amd import ops
    B, H, E, select = CASES[name]
    case = mix64.make_case(3, B, H, E, select)
    want = mix64.reference(case, softmax)
    _compare(mix64.run(ops.expert_mix_torch, case, "cpu", softmax), want, "torch")
    _compare(mix64.run(ops.expert_mix, case, "cpu", softmax), want, "op on cpu")


def test_op_on_cpu_tensors_is_the_composition_and_defaults_to_all_experts():
    from recbox_amd import ops
    case = mix64.make_case(5, 6, 8, 3, mix64.full_select(3, 2))
    a = ops.expert_mix(case["x"], case["z"])
    b = ops.expert_mix_torch(case["x"], case["z"], None, True)
    assert isinstance(a, tuple) and len(a) == 2
    for u, v in zip(a, b):
        assert torch.equal(u, v) and tuple(u.shape) == (6, 8)
    with pytest.raises(ValueError):
        ops.expert_mix(case["x"], case["z"], [[0, 1, 2]])
    with pytest.raises(IndexError):
        ops.expert_mix(case["x"], case["z"], [[0, 1, 3], [0, 1, 2]])


def test_restatement_backward_equals_autograd_in_float64():
    case = mix64.make_case(9, 5, 8, 4, [[2, 0], [0, 3, 2]])
    x = [t.double().requires_grad_() for t in case["x"]]
    z = [t.double().requires_grad_() for t in case["z"]]
    outs = [sum(torch.softmax(zt, 1)[:, j:j + 1] * x[e] for j, e in enumerate(sel)) for zt, sel in zip(z, case["select"])]
    grads = torch.autograd.grad(sum((o * u.double()).sum() for o, u in zip(outs, case["up"])), x + z, allow_unused=True)
    want = mix64.reference(case)
    for a, b in zip(grads, want["dx"] + want["dz"]):
        assert_close(a if a is not None else torch.zeros_like(b), b, 1e-12, "restatement")
    assert float(want["dx"][1].abs().max()) == 0.0


@pytest.mark.parametrize("tag", TAGS)
def test_models_match_the_reference_on_the_cpu_path(tag):
    model = mix64.check_model_against_fixture(tag, "cpu")
    fx = Fixture("rechub_multi_task")
    assert list(model.state_dict().keys()) == [str(k) for k in fx["keys"][tag]]
    for k, v in model.state_dict().items():
        assert tuple(v.shape) == tuple(fx["p_" + tag][k].shape), k


def test_state_dict_keys_are_the_reference_names():
    fx = Fixture("rechub_multi_task")
    assert {"experts.0.mlp.0.weight", "gates.1.mlp.1.running_mean", "towers.0.mlp.4.weight"} <= set(fx["keys"]["mmoe"])
    assert {"cgc_layers.0.experts_specific.3.mlp.0.weight", "cgc_layers.0.gate_shared.mlp.0.weight",
            "cgc_layers.1.gates_specific.1.mlp.1.running_var"} <= set(fx["keys"]["ple"])
    assert "cgc_layers.1.gate_shared.mlp.0.weight" not in set(fx["keys"]["ple"])
    assert {"aits.0.q_layer.weight", "aits.1.v_layer.weight", "info_gates.0.mlp.0.weight"} <= set(fx["keys"]["aitm"])
    for tag in TAGS:
        assert list(mix64.mirror(tag).state_dict().keys()) == [str(k) for k in fx["keys"][tag]], tag


def test_fixture_has_the_shapes_it_claims():
    fx = Fixture("rechub_multi_task")
    tags = fx["in"]["tags"]
    assert tags.shape == (16, 5) and (tags == 0).all(axis=1).sum() >= 2 and (tags == 0).any(axis=1).sum() > 4
    assert fx["out_mmoe"]["y"].shape == (16, 2) and fx["out_aitm"]["y"].shape == (16, 3) and fx["out_esmm"]["y"].shape == (16, 3)
    assert fx["out_ple"]["y"].shape == (16, 8)                                  # ple.py:40-41: towers without an output layer
    for tag in TAGS:
        for k, v in fx["p_" + tag].items():
            if v.dtype.kind == "f" and "running_mean" not in k:
                assert abs(v).max() > 0, k


def test_esmm_third_column_is_the_square_of_the_first():
    fx = Fixture("rechub_multi_task")
    model = mix64.mirror("esmm")
    model.load_state_dict(fx.tensors("p_esmm"), strict=True)
    y = model.train()(fx.tensors("in"))
    assert torch.equal(y[:, 2], y[:, 0] * y[:, 0])
    assert not torch.allclose(y[:, 2], y[:, 0] * y[:, 1])


def test_gate_of_another_form_runs_as_it_stands():
    """A gate whose Sequential is not Linear, BatchNorm1d, Softmax, Dropout -- or whose dropout is active -- hands its own
    output over as the weights."""
    from recbox_amd.rechub.models import multi_task
    fx = Fixture("rechub_multi_task")
    model = mix64.mirror("mmoe")
    model.load_state_dict(fx.tensors("p_mmoe"), strict=True)
    model.eval()
    x = fx.tensors("in")
    want = model(x)
    z, flag = multi_task._gate_logits(model.gates[0], torch.randn(4, model.input_dims))
    assert flag and tuple(z.shape) == (4, 3)
    model.gates[0].mlp[3].p = 0.5                                               # eval: still inactive
    assert multi_task._gate_logits(model.gates[0], torch.randn(4, model.input_dims))[1]
    model.gates[0].mlp[2] = torch.nn.Softmax(dim=-1)                            # same function, another form
    w, flag = multi_task._gate_logits(model.gates[0], torch.randn(4, model.input_dims))
    assert not flag and torch.allclose(w.sum(dim=1), torch.ones(4))
    assert_close(model(x), want, 1e-6, "mixed gate forms")


def test_header_declares_the_entry_points_and_keeps_the_version():
    with open(os.path.join(ROOT, "include", "recbox_hip.h")) as fh:
        text = fh.read()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
    assert re.search(r"#define\s+RBX_VERSION\s+124\b", text)
    assert "mmoe.py:46-57" in text and "ple.py:102-128" in text and "aitm.py:77-84" in text


def test_library_exports_and_lib_binds_them():
    from recbox_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES
        assert getattr(_lib.lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert _lib.lib.rbx_version() == 124


def _arrays(E, T, select, ptr=0x1000, stride=None, H=8):
    i32, i64, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    flat = [i for s in select for i in s]
    offs = [0]
    for s in select:
        offs.append(offs[-1] + len(s))
    return ((vp * E)(*[ptr] * E), (i64 * E)(*[H if stride is None else stride] * E), (vp * T)(*[0x1000] * T),
            (i32 * max(len(flat), 1))(*flat), (i32 * len(offs))(*offs))


def test_refusals_come_before_any_launch():
    from recbox_amd import _lib
    lib = _lib.lib
    p = 0x1000                                               # fake, never dereferenced: every refusal precedes the launch

    def fwd(H, E, select, batch=4, dtype=_lib.RBX_F32, **kw):
        x, xs, z, sel, off = _arrays(E, len(select), select, H=H, **kw)
        return lib.rbx_expert_mix_fwd(x, xs, z, sel, off, batch, H, E, len(select), 1, dtype, p, p, None)

    def bwd(H, E, select, batch=4, dtype=_lib.RBX_F32, **kw):
        x, xs, z, sel, off = _arrays(E, len(select), select, H=H, **kw)
        g = (ctypes.c_void_p * len(select))(*[p] * len(select))
        return lib.rbx_expert_mix_bwd(x, xs, z, p, g, sel, off, batch, H, E, len(select), 1, dtype, None, None, None)

    for call in (fwd, bwd):
        for H in (0, 6, 1028):
            assert call(H, 2, [[0, 1]]) == _lib.RBX_ERR_UNSUPPORTED, H
            assert _lib.last_error()
        assert call(8, 17, [list(range(16))]) == _lib.RBX_ERR_UNSUPPORTED                   # 17 experts
        assert call(8, 2, [[0, 1]] * 9) == _lib.RBX_ERR_UNSUPPORTED                         # 9 gates
        assert call(8, 2, [[0, 1], []]) == _lib.RBX_ERR_UNSUPPORTED                         # an empty selection
        assert call(8, 2, [[0, 2]]) == _lib.RBX_ERR_UNSUPPORTED                             # an index outside the experts
        assert call(8, 2, [[0, 0]]) == _lib.RBX_ERR_UNSUPPORTED                             # an expert twice in one gate
        assert call(8, 2, [[0, 1]], dtype=_lib.RBX_F64) == _lib.RBX_ERR_UNSUPPORTED         # a float64 tensor code
        assert call(8, 2, [[0, 1]], ptr=p + 4) == _lib.RBX_ERR_UNSUPPORTED                  # a misaligned expert
        assert call(8, 2, [[0, 1]], stride=18) == _lib.RBX_ERR_UNSUPPORTED                  # a stride that is no multiple of 4
        assert call(8, 2, [[0, 1]], batch=-1) == _lib.RBX_ERR_INVALID
        assert call(8, 2, [[0, 1]], batch=0) == _lib.RBX_OK                                 # empty batch: nothing launched


def test_gate_answers_on_the_edges_of_its_range():
    from recbox_amd import ops
    ok = ops.expert_mix_supported
    assert (ops.MIX_MAX_HIDDEN, ops.MIX_MAX_EXPERTS, ops.MIX_MAX_GATES, ops.MIX_MAX_SELECT) == (1024, 16, 8, 16)
    assert ok(4, 1, [[0]]) and ok(1024, 16, [list(range(16))] * 8) and ok(128, 8, n_gate=3) and ok(12, 3, n_gate=1)
    assert ok(32, 2, [[1, 0]]) and ok(64, 5, mix64.ple_select(2, 2, 1))
    assert not ok(0, 2, n_gate=1) and not ok(6, 2, n_gate=1) and not ok(1028, 2, n_gate=1) and not ok(2, 2, n_gate=1)
    assert not ok(8, 0, [[0]]) and not ok(8, 17, [list(range(16))]) and not ok(8, 17, n_gate=1)
    assert not ok(8, 2, []) and not ok(8, 2, [[0, 1]] * 9) and ok(8, 2, [[0, 1]] * 8)
    assert not ok(8, 2, [[0, 1], []]) and not ok(8, 2, [[0, 2]]) and not ok(8, 2, [[0, 0]]) and not ok(8, 2, [[-1]])
    assert not ok(8, 2, [[0, 1]], dtype=torch.float64) and not ok(8, 2, [[0, 1]], dtype=torch.float16)


def test_switch_is_spelled_like_its_neighbours():
    from recbox_amd import ops
    assert ops.config.expert_mix_fused is True or os.environ.get("RECBOX_AMD_EXPERT_MIX_FUSED") == "0"
    with open(os.path.join(ROOT, "recbox_amd", "ops.py")) as fh:
        assert 'expert_mix_fused = os.environ.get("RECBOX_AMD_EXPERT_MIX_FUSED", "1") != "0"' in fh.read()


def test_compat_names_the_models_and_their_paths_import():
    from recbox_amd import compat
    from recbox_amd.rechub.models import multi_task
    table = compat.alias_table()
    target = "recbox_amd.rechub.models.multi_task"
    for root in ("torch_rechub", "recbox.third_party.rechub"):
        assert set(table[root + ".models.multi_task"][1]) == {"SharedBottom", "ESMM", "MMOE", "PLE", "AITM", "CGC"}
        assert table[root + ".models.multi_task.shared_bottom"] == (target, ["SharedBottom"])
        assert table[root + ".models.multi_task.esmm"] == (target, ["ESMM"])
        assert table[root + ".models.multi_task.mmoe"] == (target, ["MMOE"])
        assert table[root + ".models.multi_task.ple"][0] == target and "PLE" in table[root + ".models.multi_task.ple"][1]
        assert set(table[root + ".models.multi_task.aitm"][1]) == {"AITM", "AttentionLayer"}
        assert table[root + ".models.ranking"] == ("recbox_amd.rechub.models.ranking", ["DeepFM", "DIN", "DeepFFM", "FatDeepFFM"])
    report = compat.install(prefixes=("torch_rechub", "recbox"), overlay=False)
    try:
        for root in ("torch_rechub", "recbox.third_party.rechub"):
            pkg = importlib.import_module(root + ".models.multi_task")
            for name in ("SharedBottom", "ESMM", "MMOE", "PLE", "AITM"):
                assert hasattr(pkg, name), (root, name)
                if getattr(pkg, "__recbox_amd__", False):
                    assert getattr(pkg, name) is getattr(multi_task, name)
            for leaf, name in (("shared_bottom", "SharedBottom"), ("esmm", "ESMM"), ("mmoe", "MMOE"), ("ple", "PLE"),
                               ("ple", "CGC"), ("aitm", "AITM"), ("aitm", "AttentionLayer")):
                mod = importlib.import_module("%s.models.multi_task.%s" % (root, leaf))
                assert hasattr(mod, name), (root, leaf, name)
                if getattr(mod, "__recbox_amd__", False):
                    assert getattr(mod, name) is getattr(multi_task, name)
    finally:
        compat.uninstall(report)
