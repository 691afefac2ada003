"""CPU-only checks of the training side of the ragged (CSR) lookup: rbx_embed_csr_rezero and rbx_embed_csr_sparse_update are
declared, exported and bound, and refuse -- before anything is launched, so without a GPU -- what their siblings refuse: a
NULL descriptor array, too many descriptors, a pool that keeps one slot per id, a dim no lane group holds, a rule without
its state arrays, a workspace smaller than rbx_embed_csr_bwd_workspace_size.  An empty batch and descriptors that are all
frozen return RBX_OK.  The pointers below are never dereferenced: every call returns in front of its first launch.  The
kernels are tested on the GPU: tests/test_gpu_embed_csr_optim.py."""
import ctypes
import inspect
import os
import re

import pytest

from conftest import ROOT

ENTRY_POINTS = ("rbx_embed_csr_rezero", "rbx_embed_csr_sparse_update")
FAKE = 0x10000                                     # a 16-byte aligned address nothing reads


def _bag(_lib, dim=16, pool=None, grad=True, nnz=100, vocab=50, table=FAKE):
    b = _lib.rbx_bag_t()
    b.indices, b.offsets, b.table = FAKE, FAKE, table
    b.grad = table if grad else None
    b.nnz, b.indices_stride, b.vocab = nnz, 1, vocab
    b.padding_idx, b.mask_id, b.out_off = _lib.RBX_NO_ID, _lib.RBX_NO_ID, 0
    b.dim, b.indices_dtype, b.offsets_dtype = dim, _lib.RBX_I64, _lib.RBX_I64
    b.pool = _lib.POOL_SUM if pool is None else pool
    return b


def _arr(_lib, *bags):
    return (_lib.rbx_bag_t * len(bags))(*bags)


def _opt(_lib, kind):
    return _lib.rbx_opt_t(kind, 0.01, 0.9, 0.999, 1e-8, 0.0, None)


def _states(n, *which):
    out = []
    for have in which:
        arr = (ctypes.c_void_p * n)()
        for i in range(n):
            arr[i] = FAKE if have else None
        out.append(arr)
    return out


def _update(_lib, arr, n, batch, opt, s1, s2, ws=FAKE, ws_bytes=1 << 40, clear=0):
    return _lib.lib.rbx_embed_csr_sparse_update(arr, n, batch, ws, ws_bytes, ctypes.byref(opt), s1, s2, clear, None)


def test_header_declares_and_describes_the_two_entry_points():
    text = open(os.path.join(ROOT, "include", "recbox_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(\s*const\s+rbx_bag_t\s*\*" % name, code), "%s(const rbx_bag_t* ...) is not declared" % name
        assert name in text[:text.index("typedef struct rbx_bag")], "%s is not described in the header's comment" % name
    assert re.search(r"rbx_embed_csr_sparse_update\s*\([^)]*int32_t\s+clear_grad", code)
    assert re.search(r"#define\s+RBX_VERSION\s+124\b", code)


def test_library_exports_and_lib_binds_them():
    from recbox_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert hasattr(raw, name), "librecbox_hip.so does not export %s" % name
        assert getattr(_lib.lib, name).argtypes[0] is ctypes.POINTER(_lib.rbx_bag_t)
    assert len(_lib.SIGNATURES["rbx_embed_csr_sparse_update"][1]) == 10
    assert _lib.lib.rbx_version() == 124


def test_optimisers_take_clear_grads_and_default_to_false():
    from recbox_amd import optim
    for cls in (optim.SparseSGD, optim.SparseAdagrad, optim.SparseAdam):
        assert inspect.signature(cls.__init__).parameters["clear_grads"].default is False


@pytest.mark.parametrize("call", ["rezero", "update"])
def test_descriptor_refusals_are_made_before_any_launch(call):
    from recbox_amd import _lib
    opt = _opt(_lib, _lib.OPT_SGD)

    def run(arr, n, batch=8):
        if call == "rezero":
            return _lib.lib.rbx_embed_csr_rezero(arr, n, batch, FAKE, 1 << 40, None)
        return _update(_lib, arr, n, batch, opt, None, None)

    assert run(None, 1) == _lib.RBX_ERR_INVALID and "NULL" in _lib.last_error()
    many = _arr(_lib, *[_bag(_lib) for _ in range(_lib.RBX_MAX_BAGS + 1)])
    assert run(many, _lib.RBX_MAX_BAGS + 1) == _lib.RBX_ERR_INVALID and "n_bags" in _lib.last_error()
    for pool in (_lib.POOL_NONE, _lib.POOL_CONCAT):
        assert run(_arr(_lib, _bag(_lib, pool=pool)), 1) == _lib.RBX_ERR_UNSUPPORTED and "pool" in _lib.last_error()
    for dim in (0, 1025, 2048):
        assert run(_arr(_lib, _bag(_lib, dim=dim)), 1) == _lib.RBX_ERR_UNSUPPORTED and "dim" in _lib.last_error()
    # 260 floats as 260 scalar units (a gradient that is not 16-byte aligned): no lane group holds them
    odd = _bag(_lib, dim=260)
    odd.grad = FAKE + 4
    assert run(_arr(_lib, odd), 1) == _lib.RBX_ERR_UNSUPPORTED and "too large" in _lib.last_error()


def test_missing_state_arrays_and_unknown_rules_are_invalid():
    from recbox_amd import _lib
    arr = _arr(_lib, _bag(_lib, grad=False), _bag(_lib))            # a frozen descriptor in front: its state is not looked at
    s_none, s_second, s_both = _states(2, False), _states(2, False)[0], _states(2, True, True)
    s_second[1] = FAKE
    assert _update(_lib, arr, 2, 8, _opt(_lib, _lib.OPT_ADAM), s_second, None) == _lib.RBX_ERR_INVALID
    assert "second moment" in _lib.last_error()
    assert _update(_lib, arr, 2, 8, _opt(_lib, _lib.OPT_ADAM), s_second, s_none[0]) == _lib.RBX_ERR_INVALID
    assert _update(_lib, arr, 2, 8, _opt(_lib, _lib.OPT_ADAGRAD), None, None) == _lib.RBX_ERR_INVALID
    assert "state" in _lib.last_error()
    assert _update(_lib, arr, 2, 8, _opt(_lib, 7), s_both[0], s_both[1]) == _lib.RBX_ERR_INVALID
    assert _lib.lib.rbx_embed_csr_sparse_update(arr, 2, 8, FAKE, 1 << 40, None, None, None, 0, None) == _lib.RBX_ERR_INVALID


def test_undersized_workspace_is_refused_with_its_own_code():
    from recbox_amd import _lib
    arr = _arr(_lib, _bag(_lib))
    need = _lib.lib.rbx_embed_csr_bwd_workspace_size(arr, 1, 8)
    assert need > 0
    s1, s2 = _states(1, True, True)
    for ws, nbytes in ((FAKE, need - 1), (FAKE, 0), (None, need)):
        assert _lib.lib.rbx_embed_csr_rezero(arr, 1, 8, ws, nbytes, None) == _lib.RBX_ERR_WORKSPACE
        assert "workspace" in _lib.last_error()
        for clear in (0, 1):
            assert _update(_lib, arr, 1, 8, _opt(_lib, _lib.OPT_ADAM), s1, s2, ws=ws, ws_bytes=nbytes,
                           clear=clear) == _lib.RBX_ERR_WORKSPACE
            assert "workspace" in _lib.last_error()


def test_empty_batches_and_all_frozen_descriptors_return_ok_without_a_launch():
    from recbox_amd import _lib
    s1, s2 = _states(2, True, True)
    opt = _opt(_lib, _lib.OPT_ADAM)
    live = _arr(_lib, _bag(_lib), _bag(_lib, dim=10, table=2 * FAKE))
    frozen = _arr(_lib, _bag(_lib, grad=False), _bag(_lib, dim=10, grad=False, table=2 * FAKE))
    empty = _arr(_lib, _bag(_lib, nnz=0), _bag(_lib, dim=10, nnz=0, table=2 * FAKE))
    for arr, batch in ((live, 0), (frozen, 8), (empty, 8)):
        assert _lib.lib.rbx_embed_csr_rezero(arr, 2, batch, None, 0, None) == _lib.RBX_OK
        assert _update(_lib, arr, 2, batch, opt, s1, s2, ws=None, ws_bytes=0, clear=1) == _lib.RBX_OK
    assert _update(_lib, live, 2, -1, opt, s1, s2, ws=None, ws_bytes=0) == _lib.RBX_OK
