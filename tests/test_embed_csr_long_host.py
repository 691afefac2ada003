"""Host side of the long-bag form of the ragged (CSR) lookup (no GPU): the four ``_long`` entry points and RBX_CSR_SEGMENT
are declared, exported and bound; ops.bag_long_threshold defaults to 1024 and round-trips; the workspace size depends on
static values only, is safe for nnz = 0 and never shrinks when nnz grows."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

LONG = ("rbx_embed_csr_fwd_long_workspace_size", "rbx_embed_csr_fwd_long", "rbx_embed_csr_fwd_weighted_long",
        "rbx_embed_csr_weight_grad_long")


def _header():
    return open(os.path.join(ROOT, "include", "recbox_hip.h")).read()


def test_header_declares_the_long_entry_points_and_the_segment_size():
    from recbox_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in LONG:
        assert re.search(r"\b%s\s*\(" % name, text), "%s is not declared" % name
    m = re.search(r"#define\s+RBX_CSR_SEGMENT\s+(\d+)", text)
    assert m is not None and int(m.group(1)) == 256 == _lib.CSR_SEGMENT
    for chunk in (64, 128, 256):                                            # 4 ids per lane x lane groups of 16 / 32 / 64
        assert int(m.group(1)) % chunk == 0
    for word, name in ((_lib.CSR_WS_SEGMENTS, "RBX_CSR_WS_SEGMENTS"), (_lib.CSR_WS_LONG_BAGS, "RBX_CSR_WS_LONG_BAGS")):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1)) == word


def test_library_exports_and_lib_binds_the_long_entry_points():
    from recbox_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in LONG:
        assert hasattr(raw, name), "librecbox_hip.so does not export %s" % name
        assert name in _lib.SIGNATURES and getattr(_lib.lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert _lib.SIGNATURES[LONG[0]][0] is ctypes.c_size_t


def test_bag_long_threshold_defaults_to_1024_and_round_trips():
    from recbox_amd import ops
    assert ops.bag_long_threshold() == 1024
    try:
        assert ops.bag_long_threshold(64) == 1024
        assert ops.bag_long_threshold() == 64
        assert ops.bag_long_threshold(0) == 64
        assert ops.bag_long_threshold() == 0
        with pytest.raises(ValueError):
            ops.bag_long_threshold(-1)
        assert ops.bag_long_threshold() == 0
    finally:
        ops.bag_long_threshold(1024)
    assert ops.bag_long_threshold() == 1024


def _size(nnz, batch=97, dims=(16,), threshold=64):
    from recbox_amd import _lib
    arr = (_lib.rbx_bag_t * len(dims))()
    for f, d in zip(arr, dims):
        f.nnz, f.dim, f.pool, f.vocab = nnz, d, 1, 300                      # no pointer is set: the size reads none
    return _lib.lib.rbx_embed_csr_fwd_long_workspace_size(arr, len(dims), batch, threshold)


def test_workspace_size_is_safe_for_nnz_zero_and_grows_monotonically_with_nnz():
    assert _size(0) > 0 and _size(0) == _size(63) == _size(5000, threshold=0)   # no bag can be long: the header alone
    assert _size(0, batch=0) == _size(0)
    sizes = [_size(n) for n in (0, 1, 63, 64, 65, 255, 256, 257, 1000, 4096, 100000, 1 << 20, (1 << 26) - 1)]
    assert sizes == sorted(sizes) and sizes[-1] > sizes[3] > sizes[0]
    # room for what well-formed offsets can ask: nnz / T records of 32 bytes, nnz / S + nnz / T partial rows and counts
    nnz, T, S, D = 100000, 64, 256, 16
    assert _size(nnz, batch=1 << 20) >= 256 + (nnz // T) * 32 + (nnz // S + nnz // T) * (D * 4 + 4)
    assert _size(nnz, batch=10) < _size(nnz, batch=1 << 20)                  # at most `batch` bags can be long
    assert _size(nnz, dims=(16, 132)) > _size(nnz, dims=(16, 16)) > _size(nnz)
    assert _size(nnz, batch=1 << 20, threshold=1024) < _size(nnz, batch=1 << 20, threshold=64)
    assert _size(nnz, dims=(2000,)) == 0 and _size(-1) == 0                  # refused descriptors
