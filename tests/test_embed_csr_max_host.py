"""CPU-only checks of the max pool of the ragged (CSR) lookup (RBX_POOL_MAX, torch's ``EmbeddingBag(mode="max")``): the
header declares the three entry points and the pool, the built library exports them and recbox_amd._lib binds them; every
entry point that pools a sum or a mean refuses a max descriptor and rbx_embed_csr_fwd_max refuses anything else, before a
device call; the calls that never pool accept one; the workspace size is 0-safe, monotone in nnz and no smaller than the long
workspace; the Python layer refuses weights on a max spec, max beside another pool in one plan, and the torch arguments
``recbox_amd.bag.EmbeddingBag`` does not implement.  The kernels are tested on the GPU: tests/test_gpu_embed_csr_max.py."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

ENTRY_POINTS = ("rbx_embed_csr_fwd_max", "rbx_embed_csr_fwd_max_workspace_size", "rbx_embed_csr_bwd_max")
FAKE = 0x10000                                             # a non-NULL "device pointer" no refused call may touch


def _bag(pool, nnz=100, dim=8, vocab=50, grad=True):
    from recbox_amd import _lib
    b = _lib.rbx_bag_t()
    b.indices, b.offsets, b.table, b.grad = FAKE, FAKE, FAKE, (FAKE if grad else None)
    b.nnz, b.indices_stride, b.vocab = nnz, 1, vocab
    b.padding_idx, b.mask_id, b.out_off = _lib.RBX_NO_ID, _lib.RBX_NO_ID, 0
    b.dim, b.indices_dtype, b.offsets_dtype, b.pool, b.eps, b.reserved = dim, _lib.RBX_I64, _lib.RBX_I64, pool, 0.0, 0
    return b


def _arr(*bags):
    from recbox_amd import _lib
    return (_lib.rbx_bag_t * len(bags))(*bags)


def test_header_declares_the_pool_and_the_entry_points():
    text = open(os.path.join(ROOT, "include", "recbox_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"RBX_POOL_MAX\s*=\s*6\b", code)
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(\s*const\s+rbx_bag_t\s*\*" % name, code), "%s(const rbx_bag_t* ...) is not declared" % name
        assert name in text[:text.index("typedef struct rbx_bag")], "%s is not described in the header's comment" % name
    assert re.search(r"rbx_embed_csr_fwd_max\s*\([^)]*int32_t\s*\*\s*d_argpos", code)
    assert re.search(r"rbx_embed_csr_bwd_max\s*\([^)]*const\s+int32_t\s*\*\s*d_argpos", code)
    assert "NaN" in text[text.index("Max pool (RBX_POOL_MAX"):text.index("typedef struct rbx_bag")]


def test_library_exports_and_lib_binds_the_entry_points():
    from recbox_amd import _lib, ops
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert hasattr(raw, name), "librecbox_hip.so does not export %s" % name
        assert name in _lib.SIGNATURES
        assert getattr(_lib.lib, name).argtypes[0] is ctypes.POINTER(_lib.rbx_bag_t)
    assert _lib.POOL_MAX == 6 and ops.POOL_MAX == 6


def test_every_pooling_entry_point_refuses_a_max_descriptor():
    from recbox_amd import _lib
    lib, U = _lib.lib, _lib.RBX_ERR_UNSUPPORTED
    for bags in (_arr(_bag(_lib.POOL_MAX)), _arr(_bag(_lib.POOL_SUM), _bag(_lib.POOL_MAX))):
        n, B = len(bags), 4
        w = (ctypes.c_void_p * n)(*([FAKE] * n))
        none = (ctypes.c_void_p * n)(*([None] * n))
        assert lib.rbx_embed_csr_fwd(bags, n, B, FAKE, 8, None, None, None) == U
        assert "max pool" in _lib.last_error()
        assert lib.rbx_embed_csr_fwd_long(bags, n, B, 64, FAKE, 8, None, FAKE, 1 << 20, None, None) == U
        assert lib.rbx_embed_csr_fwd_weighted(bags, n, B, none, FAKE, 8, None, None) == U
        assert lib.rbx_embed_csr_fwd_weighted(bags, n, B, w, FAKE, 8, None, None) == U
        assert lib.rbx_embed_csr_fwd_weighted_long(bags, n, B, 64, w, FAKE, 8, FAKE, 1 << 20, None, None) == U
        assert lib.rbx_embed_csr_bwd(bags, n, B, FAKE, 8, None, 0, FAKE, 1 << 30, None) == U
        assert lib.rbx_embed_csr_bwd_weighted(bags, n, B, w, FAKE, 8, 0, FAKE, 1 << 30, None) == U
        assert lib.rbx_embed_csr_weight_grad(bags, n, B, FAKE, 8, w, None, None) == U
        assert lib.rbx_embed_csr_weight_grad_long(bags, n, B, 64, FAKE, 8, w, FAKE, 1 << 20, None, None) == U


@pytest.mark.parametrize("pool", ["POOL_SUM", "POOL_SUM_ID", "POOL_MEAN_ID", "POOL_MEAN_VALUE"])
def test_the_max_entry_points_refuse_any_other_pool(pool):
    from recbox_amd import _lib
    lib = _lib.lib
    bags = _arr(_bag(_lib.POOL_MAX), _bag(getattr(_lib, pool)))
    assert lib.rbx_embed_csr_fwd_max(bags, 2, 4, 0, FAKE, 8, FAKE, 8, None, 0, None, None) == _lib.RBX_ERR_UNSUPPORTED
    assert "RBX_POOL_MAX" in _lib.last_error()
    assert lib.rbx_embed_csr_bwd_max(bags, 2, 4, FAKE, 8, FAKE, 8, 0, FAKE, 1 << 30, None) == _lib.RBX_ERR_UNSUPPORTED
    for bad in (_lib.POOL_NONE, _lib.POOL_CONCAT):
        one = _arr(_bag(bad))
        assert lib.rbx_embed_csr_fwd_max(one, 1, 4, 0, FAKE, 8, FAKE, 8, None, 0, None, None) == _lib.RBX_ERR_UNSUPPORTED
    assert lib.rbx_embed_csr_fwd_max(_arr(_bag(7)), 1, 4, 0, FAKE, 8, FAKE, 8, None, 0, None, None) == _lib.RBX_ERR_INVALID


def test_max_forward_asks_for_its_workspace_before_anything_is_launched():
    from recbox_amd import _lib
    lib = _lib.lib
    bags = _arr(_bag(_lib.POOL_MAX, nnz=5000))
    need = lib.rbx_embed_csr_fwd_max_workspace_size(bags, 1, 4, 64)
    assert lib.rbx_embed_csr_fwd_max(bags, 1, 4, 64, FAKE, 8, FAKE, 8, FAKE, need - 1, None, None) == _lib.RBX_ERR_WORKSPACE
    assert lib.rbx_embed_csr_fwd_max(bags, 1, 4, 64, FAKE, 8, FAKE, 8, None, 0, None, None) == _lib.RBX_ERR_WORKSPACE
    assert lib.rbx_embed_csr_fwd_max(bags, 1, 0, 64, None, 8, None, 8, None, 0, None, None) == _lib.RBX_OK   # no bags: nothing to do


def test_max_workspace_size_is_zero_safe_monotone_and_covers_the_long_workspace():
    from recbox_amd import _lib
    lib = _lib.lib
    assert lib.rbx_embed_csr_fwd_max_workspace_size(None, 0, 0, 64) == 0
    assert lib.rbx_embed_csr_fwd_max_workspace_size(None, 1, 4, 64) == 0
    for T in (0, 1, 64, 256, 1024):
        last = 0
        for nnz in (0, 1, 63, 64, 255, 256, 257, 1000, 4096, 100000, 1 << 20):
            for B in (0, 1, 4, 1000):
                bags = _arr(_bag(_lib.POOL_MAX, nnz=nnz, dim=10))
                got = lib.rbx_embed_csr_fwd_max_workspace_size(bags, 1, B, T)
                assert got >= lib.rbx_embed_csr_fwd_long_workspace_size(bags, 1, B, T) >= 256
                if B == 1000:
                    assert got >= last, "the size shrank when nnz grew to %d (T=%d)" % (nnz, T)
                    last = got
    # one int32 partial argpos row per segment slot on top of the long workspace
    bags = _arr(_bag(_lib.POOL_MAX, nnz=1 << 20, dim=10))
    extra = lib.rbx_embed_csr_fwd_max_workspace_size(bags, 1, 1000, 256) - lib.rbx_embed_csr_fwd_long_workspace_size(bags, 1, 1000, 256)
    slots = (1 << 20) // 256 + 1000
    assert slots * 12 * 4 <= extra < slots * 12 * 4 + 256
    assert lib.rbx_embed_csr_fwd_max_workspace_size(bags, 1, 1000, -1) == 0


def test_the_calls_that_never_pool_accept_max_descriptors():
    from recbox_amd import _lib
    lib = _lib.lib
    mx, sm = _arr(_bag(_lib.POOL_MAX, nnz=1000)), _arr(_bag(_lib.POOL_SUM_ID, nnz=1000))
    need = lib.rbx_embed_csr_bwd_workspace_size(mx, 1, 16)
    assert need > 0 and need == lib.rbx_embed_csr_bwd_workspace_size(sm, 1, 16)
    mixed = _arr(_bag(_lib.POOL_SUM, nnz=10), _bag(_lib.POOL_MAX, nnz=1000))
    assert lib.rbx_embed_csr_bwd_workspace_size(mixed, 2, 16) > 0
    # too small a workspace: each of them gets past the descriptor checks and stops at the size
    for call in (lambda ws, n: lib.rbx_embed_csr_sort(mx, 1, 16, ws, n, None, None),
                 lambda ws, n: lib.rbx_embed_csr_sort_weighted(mx, 1, 16, ws, n, None, None),
                 lambda ws, n: lib.rbx_embed_csr_rezero(mx, 1, 16, ws, n, None),
                 lambda ws, n: lib.rbx_embed_csr_bwd_max(mx, 1, 16, FAKE, 8, FAKE, 8, 0, ws, n, None)):
        assert call(FAKE, need - 1) == _lib.RBX_ERR_WORKSPACE, _lib.last_error()
    opt = _lib.rbx_opt_t()
    opt.kind, opt.lr = _lib.OPT_SGD, 0.1
    none = (ctypes.c_void_p * 1)(None)
    assert lib.rbx_embed_csr_sparse_update(mx, 1, 16, FAKE, need - 1, ctypes.byref(opt), none, none, 0, None) == _lib.RBX_ERR_WORKSPACE
    # the padded lookup keeps refusing pool 6 the way it did
    f = _lib.rbx_field_t()
    f.ids, f.table, f.vocab, f.dim, f.seq_len, f.ids_dtype, f.kind, f.pool = FAKE, FAKE, 50, 8, 4, _lib.RBX_I64, 0, _lib.POOL_MAX
    f.padding_idx = f.mask_id = _lib.RBX_NO_ID
    assert lib.rbx_embed_fwd((_lib.rbx_field_t * 1)(f), 1, 4, FAKE, 8, None, None, None) == _lib.RBX_ERR_INVALID
    assert "bad pool mode" in _lib.last_error()
    assert lib.rbx_embed_bwd_workspace_size((_lib.rbx_field_t * 1)(f), 1, 4) == 0


def _carrier(weights=None):
    from recbox_amd import ops
    bags = ops.Bags.__new__(ops.Bags)                                      # a carrier built around the GPU checks
    bags.indices, bags.offsets, bags.weights = torch.tensor([1, 2, 3]), torch.tensor([0, 1, 3]), weights
    return bags


def test_python_refusals_that_raise_before_any_device_call():
    from recbox_amd import ops
    from recbox_amd.bag import EmbeddingBag
    plan = ops.BagPlan([ops.BagSpec("peak", 4, 0, 0, ops.POOL_MAX, 5), ops.BagSpec("peak2", 4, 4, 0, ops.POOL_MAX, 5)])
    assert plan.is_max and not plan.needs_row_scale
    with pytest.raises(NotImplementedError, match="peak2.*per.sample weights"):
        plan.bind_inputs([_carrier(), _carrier(torch.ones(3))])
    for other in (ops.POOL_SUM, ops.POOL_SUM_ID, ops.POOL_MEAN_ID, ops.POOL_MEAN_VALUE):
        for order in (0, 1):
            specs = [ops.BagSpec("peak", 4, 0, 0, ops.POOL_MAX, 5), ops.BagSpec("total", 4, 4, 0, other, 5)]
            with pytest.raises(NotImplementedError, match="total.*embed_bags call of their own"):
                ops.BagPlan(specs[::-1] if order else specs)
    assert not ops.BagPlan([ops.BagSpec("total", 4, 0, 0, ops.POOL_SUM, 5)]).is_max
    for kw in ({"max_norm": 1.0}, {"scale_grad_by_freq": True}, {"sparse": True}):
        with pytest.raises(NotImplementedError, match=list(kw)[0].split("_")[0]):
            EmbeddingBag(10, 4, **kw)
    with pytest.raises(ValueError, match="mode"):
        EmbeddingBag(10, 4, mode="min")
    for mode in ("mean", "max"):
        m = EmbeddingBag(10, 4, mode=mode)
        with pytest.raises(NotImplementedError, match="per_sample_weights"):
            m(torch.tensor([1, 2, 3]), torch.tensor([0, 1]), per_sample_weights=torch.ones(3))
    m = EmbeddingBag(10, 4, mode="max", padding_idx=-1)
    assert m.padding_idx == 9 and m._plan.is_max and float(m.weight.detach()[9].abs().sum()) == 0.0
    with pytest.raises(ValueError, match="offsets has to be None"):
        m(torch.zeros(2, 3, dtype=torch.long), torch.tensor([0, 1]))
    with pytest.raises(ValueError, match="offsets"):
        m(torch.zeros(3, dtype=torch.long))
    with pytest.raises(RuntimeError, match="GPU"):                         # the mapping reached ops.Bags
        m(torch.tensor([1, 2, 3]), torch.tensor([0, 1]))
