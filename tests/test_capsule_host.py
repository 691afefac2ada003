"""Multi-interest routing (csrc/rbx_capsule.hip), the parts that need no GPU: the C ABI's entry points are declared, exported
and bound, the version stays put; the float64 restatement of tests/capsule64.py reproduces the live reference's MIND and
ComirecDR user towers (tests/golden/rechub_multi_interest.npz, written by tests/gen_golden_multi_interest.py), which pins the
restatement the GPU tests measure against; the mirrors carry the reference's state_dict keys; the gate answers on its edges;
the ops refuse CPU tensors; the compat paths import."""
import ctypes
import importlib
import os
import re

import pytest
import torch

import capsule64
from conftest import Fixture, assert_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["rbx_capsule_hat", "rbx_capsule_route_fwd", "rbx_capsule_route_bwd", "rbx_capsule_bilinear_dx",
         "rbx_capsule_bilinear_dw_workspace_size", "rbx_capsule_bilinear_dw", "rbx_capsule_route_supported",
         "rbx_capsule_dw_split"]
B, L, D, K = 16, 6, 8, 3


def test_header_declares_the_entry_points_and_keeps_the_version():
    with open(os.path.join(ROOT, "include", "recbox_hip.h")) as fh:
        text = fh.read()
    for name in NAMES:
        assert re.search(r"\b(int|int32_t|size_t)\s+%s\s*\(" % name, text), name
    assert re.search(r"#define\s+RBX_VERSION\s+124\b", text)
    assert "layers.py:588-643" in text                      # the entries cite what they replace


def test_library_exports_and_lib_binds_them():
    from recbox_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES
        assert getattr(_lib.lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert _lib.lib.rbx_version() == 124


def test_refusals_come_before_any_launch():
    from recbox_amd import _lib
    lib = _lib.lib
    p = 0x1000                                               # fake, never dereferenced: every refusal precedes the launch
    for dim in (6, 132, 0):
        assert lib.rbx_capsule_hat(p, 64, 8, p, 4, 7, dim, 4, p, None) == _lib.RBX_ERR_UNSUPPORTED, dim
        assert _lib.last_error()
        assert lib.rbx_capsule_route_fwd(p, 64, 8, 8, p, _lib.RBX_I64, 7, 1, None, 4, 4, 7, dim, 2, p, p, p,
                                         None) == _lib.RBX_ERR_UNSUPPORTED
        assert lib.rbx_capsule_bilinear_dx(p, p, 64, 0, p, 4, 7, dim, 4, p, None) == _lib.RBX_ERR_UNSUPPORTED
        assert lib.rbx_capsule_bilinear_dw(p, 64, 8, p, 64, 0, p, 4, 7, dim, 4, p, None, 0, None) == _lib.RBX_ERR_UNSUPPORTED
    assert lib.rbx_capsule_route_fwd(p, 64, 8, 8, p, _lib.RBX_I64, 7, 1, None, 4, 4, 7, 8, 3, p, p, p,
                                     None) == _lib.RBX_ERR_UNSUPPORTED                                  # updates = 3
    assert lib.rbx_capsule_route_fwd(p, 64, 8, 8, p, _lib.RBX_F64, 7, 1, None, 4, 4, 7, 8, 2, p, p, p,
                                     None) == _lib.RBX_ERR_UNSUPPORTED                                  # a float64 mask
    assert lib.rbx_capsule_route_fwd(p, 64, 8, 8, p, _lib.RBX_I64, 7, 1, None, 4, 4, 300, 64, 2, p, p, p,
                                     None) == _lib.RBX_ERR_UNSUPPORTED                                  # the slice does not fit
    assert lib.rbx_capsule_hat(p, 64, 8, p, 4, 7, 8, 33, p, None) == _lib.RBX_ERR_UNSUPPORTED             # 33 interests
    assert lib.rbx_capsule_hat(p, 62, 8, p, 4, 7, 8, 4, p, None) == _lib.RBX_ERR_UNSUPPORTED              # stride % 4
    assert lib.rbx_capsule_hat(p, 64, 8, p, 0, 7, 8, 4, p, None) == _lib.RBX_OK                           # empty batch


def test_workspace_size_follows_the_split():
    from recbox_amd import _lib, ops
    split = ops.CAPSULE_DW_SPLIT
    assert split == _lib.lib.rbx_capsule_dw_split() and split >= 128
    size = _lib.lib.rbx_capsule_bilinear_dw_workspace_size
    assert size(split, 3, 16, 2) == 0                        # one split stores dW directly
    assert size(split + 1, 3, 16, 2) == 2 * 3 * 32 * 16 * 4
    assert size(4 * split, 50, 64, 4) == 4 * 50 * 256 * 64 * 4


def test_gate_answers_on_its_edges():
    from recbox_amd import ops
    assert ops.capsule_supported(200, 64, 4) and ops.capsule_supported(50, 128, 8) and ops.capsule_supported(1, 4, 1)
    assert ops.capsule_supported(7, 16, 4, routing_times=1)
    assert not ops.capsule_supported(7, 6, 4)                # D = 6
    assert not ops.capsule_supported(7, 132, 4)              # D = 132
    assert not ops.capsule_supported(7, 16, 4, dtype=torch.float64)
    assert not ops.capsule_supported(7, 16, 4, routing_times=0)
    assert not ops.capsule_supported(300, 64, 4)             # an [L, D] slice beyond the routing kernel's LDS
    assert not ops.capsule_supported(7, 16, 33)


def test_ops_refuse_cpu_tensors():
    from recbox_amd import ops
    x, w = torch.randn(4, 7, 16), torch.randn(1, 7, 64, 16)
    mask = torch.ones(4, 7, dtype=torch.long)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.capsule_bilinear(x, w)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.capsule_route(torch.randn(4, 7, 64), mask, 4)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.capsule_bilinear_route(x, w, mask, 4)


def test_stop_grad_false_raises_and_w_is_initialised():
    from recbox_amd.rechub.basic.layers import CapsuleNetwork
    cap = CapsuleNetwork(16, 7, bilinear_type=2, interest_num=4)
    assert set(cap.state_dict().keys()) == {"w", "relu.0.weight"} and tuple(cap.w.shape) == (1, 7, 64, 16)
    assert torch.isfinite(cap.w).all() and 0 < cap.w.abs().max() < 0.1          # N(0, 0.01^2), never uninitialised memory
    assert set(CapsuleNetwork(16, 7, bilinear_type=0).state_dict().keys()) == {"linear.weight", "relu.0.weight"}
    assert tuple(CapsuleNetwork(16, 7, bilinear_type=1, interest_num=4).linear.weight.shape) == (64, 16)
    cap.stop_grad = False
    with pytest.raises(NotImplementedError):
        cap(torch.randn(2, 7, 16), torch.ones(2, 7, dtype=torch.long))


def _user_tower64(fx, tag, btype):
    """The user tower restated in float64: normalize(cat(user row, capsules) @ convert_user_weight)."""
    sd = {k: v.double() for k, v in fx.tensors("p_" + tag).items()}
    x = fx.tensors("in")
    hist = x["hist_item_id"]
    item = sd["embedding.embed_dict.item_id.weight"]
    weight = sd["capsule.w"] if btype == 2 else sd["capsule.linear.weight"]
    init = fx.tensors("extra")["mind_start"].double() if btype == 0 else None
    caps = capsule64.capsule_forward(item[hist], (hist > 0).long(), weight, btype, K, 3, init)
    user = sd["embedding.embed_dict.user_id.weight"][x["user_id"]].unsqueeze(1).expand(B, K, D)
    return torch.nn.functional.normalize(torch.cat([user, caps], dim=-1) @ sd["convert_user_weight"], p=2, dim=-1)


@pytest.mark.parametrize("tag,btype", [("mind", 0), ("comirec", 2)])
def test_float64_restatement_reproduces_the_reference(tag, btype):
    fx = Fixture("rechub_multi_interest")
    assert (fx["in"]["hist_item_id"] == 0).all(axis=1).any()                    # an empty history is in the fixture
    assert tuple(fx["out_" + tag]["y"].shape) == (B, D)
    assert_close(_user_tower64(fx, tag, btype), fx["out_" + tag]["user"], 1e-5, "user " + tag)


def _mirror(tag):
    from recbox_amd.rechub.basic.features import SequenceFeature, SparseFeature
    from recbox_amd.rechub.models.matching import MIND, ComirecDR
    user = [SparseFeature("user_id", vocab_size=11, embed_dim=D)]
    hist = [SequenceFeature("hist_item_id", vocab_size=23, embed_dim=D, pooling="concat", shared_with="item_id")]
    item = [SparseFeature("item_id", vocab_size=23, embed_dim=D)]
    neg = [SequenceFeature("neg_items", vocab_size=23, embed_dim=D, pooling="concat", shared_with="item_id")]
    return (MIND if tag == "mind" else ComirecDR)(user, hist, item, neg, max_length=L, interest_num=K)


@pytest.mark.parametrize("tag", ["mind", "comirec"])
def test_mirrors_carry_the_reference_state_dict_keys(tag):
    fx = Fixture("rechub_multi_interest")
    model = _mirror(tag)
    assert set(model.state_dict().keys()) == set(fx["p_" + tag].keys())
    for k, v in model.state_dict().items():
        assert tuple(v.shape) == tuple(fx["p_" + tag][k].shape), k
    model.load_state_dict(fx.tensors("p_" + tag), strict=True)


def test_compat_names_the_models_and_their_paths_import():
    from recbox_amd import compat
    table = compat.alias_table()
    for root in ("torch_rechub", "recbox.third_party.rechub"):
        assert table[root + ".models.matching.mind"] == ("recbox_amd.rechub.models.matching", ["MIND"])
        assert table[root + ".models.matching.comirec"] == ("recbox_amd.rechub.models.matching", ["ComirecDR"])
        assert {"MIND", "ComirecDR", "DSSM", "YoutubeDNN", "SASRec"} <= set(table[root + ".models.matching"][1])
    report = compat.install(prefixes=("torch_rechub",), overlay=False)
    try:
        from recbox_amd.rechub.basic import layers as ours
        from recbox_amd.rechub.models import matching
        for path, name in (("torch_rechub.models.matching.mind", "MIND"), ("torch_rechub.models.matching.comirec", "ComirecDR")):
            mod = importlib.import_module(path)
            if getattr(mod, "__recbox_amd__", False):
                assert getattr(mod, name) is getattr(matching, name)
        layers = importlib.import_module("torch_rechub.basic.layers")
        if getattr(layers, "__recbox_amd__", False):
            assert layers.CapsuleNetwork is ours.CapsuleNetwork
    finally:
        compat.uninstall(report)
