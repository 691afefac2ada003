"""Field-aware FM (csrc/rbx_ffm.hip), the parts that need no GPU: the C ABI's four entry points are declared, exported and
bound, the version stays put; the float64 restatement of tests/ffm64.py reproduces the live reference's DeepFFM and
FatDeepFFM (tests/golden/rechub_deepffm.npz, written by tests/gen_golden_deepffm.py) in outputs and gradients, which pins the
restatement the GPU tests measure against; the mirrors carry the reference's state_dict keys; the op refuses CPU tensors;
the compat paths import."""
import ctypes
import importlib
import os
import re

import pytest
import torch

import ffm64
from conftest import Fixture, assert_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["rbx_ffm_fwd", "rbx_ffm_bwd_workspace_size", "rbx_ffm_sort", "rbx_ffm_bwd"]
F, D = 4, 8
VOCABS = [3, 5, 7, 11]
FEATS = ["C%d" % i for i in range(F)]


def test_header_declares_the_entry_points_and_keeps_the_version():
    with open(os.path.join(ROOT, "include", "recbox_hip.h")) as fh:
        text = fh.read()
    for name in NAMES:
        assert re.search(r"\b(int|size_t)\s+%s\s*\(" % name, text), name
    assert re.search(r"#define\s+RBX_VERSION\s+124\b", text)


def test_library_exports_and_lib_binds_them():
    from recbox_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES
        assert getattr(_lib.lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert _lib.lib.rbx_version() == 124


def _desc(dims, vocabs, pad=None, same_table=False, stride=0):
    """Descriptors over fake (never dereferenced) 16-byte aligned addresses: the refusals come before any launch."""
    from recbox_amd import _lib
    arr = (_lib.rbx_field_t * len(dims))()
    for i, (f, d, v) in enumerate(zip(arr, dims, vocabs)):
        f.ids, f.table, f.grad = 0x1000, 0x100000 * (1 if same_table else i + 1), 0
        f.ids_stride_b, f.vocab, f.dim, f.seq_len, f.ids_dtype = 1, v, d, 1, _lib.RBX_I64
        f.kind, f.pool = _lib.FIELD_CATEGORICAL, _lib.POOL_NONE
        f.padding_idx = _lib.RBX_NO_ID if pad is None else pad
        f.mask_id = _lib.RBX_NO_ID
        f.table_stride = stride
    return arr


@pytest.mark.parametrize("case", ["D=6", "D=256", "F*D=1040", "F=1", "padding_idx", "shared table", "table_stride"])
def test_refusals_come_before_any_launch(case):
    from recbox_amd import _lib
    n, kw, d = 4, {}, 8
    if case == "D=6":
        d = 6
    elif case == "D=256":
        d = 256
    elif case == "F*D=1040":
        n, d = 13, 80
    elif case == "F=1":
        n = 1
    elif case == "padding_idx":
        kw["pad"] = 0
    elif case == "shared table":
        kw["same_table"] = True
    else:
        kw["stride"] = 32
    arr = _desc([d] * n, [n * 3] * n, **kw)
    assert _lib.lib.rbx_ffm_fwd(arr, n, 4, 0, None, 0, None, None) == _lib.RBX_ERR_UNSUPPORTED, case
    assert _lib.last_error()
    assert _lib.lib.rbx_ffm_sort(arr, n, 4, None, 0, None, None) == _lib.RBX_ERR_UNSUPPORTED, case
    assert _lib.lib.rbx_ffm_bwd(arr, n, 4, 0, None, 0, 0, None, 0, None) == _lib.RBX_ERR_UNSUPPORTED, case
    assert _lib.lib.rbx_ffm_bwd_workspace_size(arr, n, 4) == 0


def test_empty_batch_and_workspace_size():
    from recbox_amd import _lib
    arr = _desc([8] * 4, [12, 20, 28, 44])
    assert _lib.lib.rbx_ffm_fwd(arr, 4, 0, 0, None, 0, None, None) == _lib.RBX_OK
    for f in arr:
        f.grad = f.table
    last = 0
    for batch in (1, 37, 4096, 65536):
        now = _lib.lib.rbx_ffm_bwd_workspace_size(arr, 4, batch)
        assert last < now < (1 << 34), (batch, now)
        last = now


def _state(fx, tag, requires_grad):
    sd = {}
    for k, v in fx.tensors("p_" + tag).items():
        sd[k] = v.double().requires_grad_(True) if (requires_grad and v.is_floating_point() and "running" not in k) else v
    return sd


@pytest.mark.parametrize("tag", ["deep", "fat"])
def test_float64_restatement_reproduces_the_reference(tag):
    fx = Fixture("rechub_deepffm")
    x = fx.tensors("in")
    sd = _state(fx, tag, True)
    y = ffm64.deepffm_forward(sd, x, FEATS, FEATS, fat=(tag == "fat"))
    assert_close(y, fx["out_" + tag]["y"], 1e-5, "y " + tag)
    y.sum().backward()
    for name, want in fx["g_" + tag].items():
        got = sd[name].grad if sd[name].grad is not None else torch.zeros_like(sd[name])
        assert_close(got, want, 1e-5, "grad " + name)


def _mirror(tag, pad=None):
    from recbox_amd.rechub.basic.features import SparseFeature
    from recbox_amd.rechub.models.ranking import DeepFFM, FatDeepFFM
    linear = [SparseFeature(n, vocab_size=v, embed_dim=1) for n, v in zip(FEATS, VOCABS)]
    cross = [SparseFeature(n, vocab_size=v * F, embed_dim=D, padding_idx=pad if i == 1 else None)
             for i, (n, v) in enumerate(zip(FEATS, VOCABS))]
    mlp = {"dims": [16, 8], "dropout": 0.0, "activation": "relu"}
    return FatDeepFFM(linear, cross, D, 2, mlp) if tag == "fat" else DeepFFM(linear, cross, D, mlp)


@pytest.mark.parametrize("tag", ["deep", "fat"])
def test_mirrors_carry_the_reference_state_dict_keys(tag):
    fx = Fixture("rechub_deepffm")
    model = _mirror(tag)
    assert set(model.state_dict().keys()) == set(fx["p_" + tag].keys())
    for k, v in model.state_dict().items():
        assert tuple(v.shape) == tuple(fx["p_" + tag][k].shape), k
    model.load_state_dict(fx.tensors("p_" + tag), strict=True)


def test_ffm_layer_matches_the_restatement_on_a_gathered_block():
    from recbox_amd.rechub.basic.layers import FFM
    g = torch.Generator().manual_seed(3)
    x = torch.randn(5, 4, 4, 8, generator=g, dtype=torch.float64)
    want = torch.stack([x[:, i, j] * x[:, j, i] for i, j in ffm64.pairs(4)], dim=1)
    assert torch.equal(FFM(4, reduce_sum=False)(x), want)
    assert torch.equal(FFM(4, reduce_sum=True)(x), want.sum(-1, keepdim=True))
    assert "_pair_i" not in FFM(4).state_dict()


def test_ffm_cross_refuses_cpu_tensors():
    from recbox_amd import ops
    tables = [torch.randn(3 * 2, 8) for _ in range(2)]
    ids = [torch.zeros(4, dtype=torch.long) for _ in range(2)]
    with pytest.raises(RuntimeError, match="GPU"):
        ops.ffm_cross(tables, ids)
    assert not ops.ffm_supported(tables, ids)
    assert ops.config.ffm_fused is (os.environ.get("RECBOX_AMD_FFM_FUSED", "1") != "0")


def test_compat_paths_import():
    from recbox_amd import compat
    table = compat.alias_table()
    for root in ("torch_rechub", "recbox.third_party.rechub"):
        target, names = table[root + ".models.ranking.deepffm"]
        assert target == "recbox_amd.rechub.models.ranking" and set(names) == {"DeepFFM", "FatDeepFFM"}
        assert {"DeepFFM", "FatDeepFFM"} <= set(table[root + ".models.ranking"][1])
        assert table[root + ".basic.layers"] == ("recbox_amd.rechub.basic.layers", None)
    report = compat.install(prefixes=("torch_rechub",), overlay=False)
    try:
        mod = importlib.import_module("torch_rechub.models.ranking.deepffm")
        layers = importlib.import_module("torch_rechub.basic.layers")
        from recbox_amd.rechub.basic import layers as ours
        from recbox_amd.rechub.models import ranking
        if getattr(mod, "__recbox_amd__", False):
            assert mod.DeepFFM is ranking.DeepFFM and mod.FatDeepFFM is ranking.FatDeepFFM
        if getattr(layers, "__recbox_amd__", False):
            assert layers.FFM is ours.FFM and layers.CEN is ours.CEN
    finally:
        compat.uninstall(report)
