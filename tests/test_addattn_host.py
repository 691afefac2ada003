"""The fused additive attention pooling (csrc/rbx_addattn.hip), the parts that need no GPU: the C ABI's entry points are
declared with what they replace, exported and bound, the version stays put; the gate answers on its edges and refusals precede
any launch; the composition ``ops.additive_attn_pool_torch`` equals the float64 restatement of tests/addattn64.py on the CPU;
that restatement's STAMP reproduces the live reference (tests/golden/rechub_stamp.npz, written by tests/gen_golden_stamp.py),
which pins what the GPU tests measure against; the mirror carries the reference's state_dict keys; the compat paths import."""
import ctypes
import importlib
import os
import re

import pytest
import torch

import addattn64
from conftest import Fixture, assert_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["rbx_addattn_supported", "rbx_addattn_fwd", "rbx_addattn_bwd_workspace_size", "rbx_addattn_bwd"]
SHAPES = [(1, 4, 4), (7, 16, 16), (17, 20, 12), (50, 64, 64), (20, 100, 100), (200, 128, 128)]
B, L, D, V = 16, 6, 8, 23


def test_header_declares_the_entry_points_and_keeps_the_version():
    with open(os.path.join(ROOT, "include", "recbox_hip.h")) as fh:
        text = fh.read()
    for name in NAMES:
        assert re.search(r"\b(int|size_t)\s+%s\s*\(" % name, text), name
    assert re.search(r"#define\s+RBX_VERSION\s+124\b", text)
    assert "narm.py:60-68" in text and "stamp.py:69-72" in text                   # the entries cite what they replace


def test_library_exports_and_lib_binds_them():
    from recbox_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES
        assert getattr(_lib.lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert _lib.lib.rbx_version() == 124


def test_gate_edges():
    from recbox_amd import ops
    for L_, D_, H_ in SHAPES:
        assert ops.additive_attn_supported(D_, H_, L_)
    assert ops.additive_attn_supported(128, 4, 1) and ops.additive_attn_supported(4, 128, 100000)
    for D_, H_, L_ in [(6, 16, 7), (16, 6, 7), (132, 16, 7), (16, 132, 7), (0, 16, 7), (16, 0, 7), (16, 16, 0), (2, 2, 1)]:
        assert not ops.additive_attn_supported(D_, H_, L_), (D_, H_, L_)


def test_refusals_come_before_any_launch():
    """NULL-free garbage pointers are never dereferenced on the host, and nothing is launched: every call fails first."""
    from recbox_amd import _lib
    lib, p = _lib.lib, ctypes.c_void_p(4096)

    def fwd(batch=4, seq=7, dim=16, hid=16, dtype=_lib.RBX_F32, sb=112, sl=16, mask_dt=_lib.RBX_I64, x=p):
        return lib.rbx_addattn_fwd(x, sb, sl, p, None, p, p, mask_dt, 0.0, batch, seq, dim, hid, dtype, p, p, None)
    assert fwd(dim=6) == _lib.RBX_ERR_UNSUPPORTED and fwd(hid=132) == _lib.RBX_ERR_UNSUPPORTED
    assert fwd(seq=0) == _lib.RBX_ERR_UNSUPPORTED
    assert fwd(dtype=_lib.RBX_F64) == _lib.RBX_ERR_UNSUPPORTED
    assert fwd(sl=18) == _lib.RBX_ERR_UNSUPPORTED and fwd(sb=113) == _lib.RBX_ERR_UNSUPPORTED
    assert fwd(x=ctypes.c_void_p(4100)) == _lib.RBX_ERR_UNSUPPORTED
    assert fwd(mask_dt=_lib.RBX_F64) == _lib.RBX_ERR_UNSUPPORTED
    assert fwd(batch=-1) == _lib.RBX_ERR_INVALID
    assert fwd(batch=0) == _lib.RBX_OK                                            # an empty batch launches nothing
    assert lib.rbx_addattn_bwd(p, 16, p, 112, 16, p, None, p, None, 0, p, 0.0, 4, 7, 16, 16, _lib.RBX_F32, p, p, p, None, None,
                               0, None) == _lib.RBX_ERR_WORKSPACE
    assert lib.rbx_addattn_bwd(p, 18, p, 112, 16, p, None, p, None, 0, p, 0.0, 4, 7, 16, 16, _lib.RBX_F32, p, p, p, None, p,
                               1 << 20, None) == _lib.RBX_ERR_UNSUPPORTED
    assert lib.rbx_addattn_bwd_workspace_size(0, 16) == 0
    assert lib.rbx_addattn_bwd_workspace_size(37, 16) == 37 * 16 * 4
    assert lib.rbx_addattn_bwd_workspace_size(1 << 20, 128) == lib.rbx_addattn_bwd_workspace_size(1 << 16, 128)


@pytest.mark.parametrize("B_", [1, 37])
@pytest.mark.parametrize("L_,D_,H_", SHAPES)
def test_composition_matches_the_float64_restatement_on_cpu(L_, D_, H_, B_):
    """``ops.additive_attn_pool`` on CPU tensors IS the composition: within a tenth of the tolerance the GPU tests use."""
    from recbox_amd import ops
    case = addattn64.make_case(B_, L_, D_, H_)
    for eps in (0.0, 1e-12):
        ref = addattn64.reference(case, eps=eps)
        for fn in (ops.additive_attn_pool_torch, ops.additive_attn_pool):
            got = addattn64.run(fn, case, eps=eps)
            for n in addattn64.NAMES:
                assert_close(got[n], ref[n], 1e-5, "%s eps=%g" % (n, eps))
    ref = addattn64.reference(case, use_ctx=False, masked=False)
    got = addattn64.run(ops.additive_attn_pool_torch, case, use_ctx=False, masked=False)
    for n in addattn64.NAMES:
        if ref[n] is not None:
            assert_close(got[n], ref[n], 1e-5, n + " no ctx, no mask")


def test_composition_edge_rows():
    """One valid position: alpha = 1; none: NaN with eps = 0 (the plain division) and zeros with eps > 0."""
    from recbox_amd import ops
    case = addattn64.make_case(3, 5, 8, 8)
    mask = torch.tensor([[1, 0, 0, 0, 0], [0, 0, 0, 0, 0], [1, 1, 1, 1, 1]])
    out, alpha = ops.additive_attn_pool_torch(case["x"], case["w"], case["ctx"], case["v"], mask, 0.0)
    assert alpha[0].tolist() == [1.0, 0.0, 0.0, 0.0, 0.0] and torch.equal(out[0], case["x"][0, 0])
    assert torch.isnan(alpha[1]).all() and torch.isnan(out[1]).all()
    out, alpha = ops.additive_attn_pool_torch(case["x"], case["w"], case["ctx"], case["v"], mask, 1e-12)
    assert (alpha[1] == 0).all() and (out[1] == 0).all()
    assert not alpha.requires_grad


def test_float64_restatement_reproduces_the_reference_stamp():
    fx = Fixture("rechub_stamp")
    ids = fx.tensors("in")["session"]
    lengths = (ids != 0).sum(1)
    assert tuple(ids.shape) == (B, L) and lengths.min() == 1 and lengths.max() == L
    assert fx["p_stamp"]["b_a"].any() and fx["p_stamp"]["item_emb.weight"][0].any()
    sd = {k: v.double().requires_grad_() for k, v in fx.tensors("p_stamp").items()}
    z = addattn64.stamp_scores(sd, ids)
    assert tuple(z.shape) == (B, V)
    assert_close(z, fx["out_stamp"]["z"], 1e-6, "stamp z")
    z.sum().backward()
    assert set(fx["g_stamp"]) == set(sd)
    for k, p in sd.items():
        ref = torch.from_numpy(fx["g_stamp"][k]).double()
        assert_close(p.grad, ref, 1e-6 * max(1.0, ref.abs().max().item()), "stamp grad " + k)


def _mirror():
    from recbox_amd.rechub.basic.features import SequenceFeature
    from recbox_amd.rechub.models.matching import STAMP
    return STAMP(SequenceFeature("session", vocab_size=V, embed_dim=D, pooling="concat"), 0.3, 0.5)


def test_mirror_carries_the_reference_state_dict():
    fx = Fixture("rechub_stamp")
    model = _mirror()
    assert type(model.item_emb) is torch.nn.Embedding and model.item_emb.padding_idx == 0
    assert model.item_emb.weight[0].abs().sum() > 0                               # normal_ overwrote the padding row, as there
    assert model.b_a.abs().sum() == 0 and model.f_s[1].bias.abs().sum() == 0
    assert [n for n, _ in model.named_parameters()] == ["w_0", "w_1_t", "w_2_t", "w_3_t", "b_a", "item_emb.weight",
                                                        "f_s.1.weight", "f_s.1.bias", "f_t.1.weight", "f_t.1.bias"]
    model.load_state_dict(fx.tensors("p_stamp"), strict=True)
    with pytest.raises(RuntimeError):
        model({"session": fx.tensors("in")["session"]})                           # GPU-only, like NARM


def test_compat_lists_stamp():
    from recbox_amd import compat
    from recbox_amd.rechub.models import matching
    table = compat.alias_table()
    for root in ("torch_rechub", "recbox.third_party.rechub"):
        assert table[root + ".models.matching.stamp"] == ("recbox_amd.rechub.models.matching", ["STAMP"])
        assert "STAMP" in table[root + ".models.matching"][1]
    report = compat.install(prefixes=("torch_rechub",))
    try:
        assert importlib.import_module("torch_rechub.models.matching.stamp").STAMP is matching.STAMP
        assert importlib.import_module("torch_rechub.models.matching").STAMP is matching.STAMP
    finally:
        compat.uninstall(report)
