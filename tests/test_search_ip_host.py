"""CPU-only checks of the fused inner-product search (rbx_search_ip): the header declares the two entry
points, the built library exports them and recbox_amd._lib binds them, RBX_VERSION did not move; the workspace size is 0
exactly for the shapes the fused path does not serve (rbx_topk's sample-rank rule, k > 1024, 2^31 items, dim > 512) and
the call refuses them before touching the device; ops.search_ip refuses CPU tensors.  The kernels are tested on the GPU:
tests/test_gpu_search_ip.py."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT
from retrieval_exact import sample_rank                    # rbx_topk's sample-rank rule: one restatement for all tests

ENTRY_POINTS = ("rbx_search_ip_workspace_size", "rbx_search_ip")
FAKE = 0x10000                                             # a non-NULL "device pointer" no refused call may touch


def test_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "recbox_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"size_t\s+rbx_search_ip_workspace_size\s*\(\s*int64_t\s+rows\s*,\s*int64_t\s+n_items\s*,\s*int32_t\s+dim\s*,"
                     r"\s*int32_t\s+k\s*\)", code)
    assert re.search(r"int\s+rbx_search_ip\s*\(\s*const\s+float\s*\*\s*d_users[^)]*int32_t\s*\*\s*d_row_state[^)]*void\s*\*\s*stream\s*\)",
                     code)
    assert re.search(r"#define\s+RBX_VERSION\s+124\b", code)


def test_library_exports_and_lib_binds_the_entry_points():
    from recbox_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert hasattr(raw, name), "librecbox_hip.so does not export %s" % name
        assert name in _lib.SIGNATURES
        assert getattr(_lib.lib, name).argtypes is not None
    assert _lib.lib.rbx_version() == 124


@pytest.mark.parametrize("rows,n,dim,k", [(5, 16384, 16, 500), (5, 100, 16, 10), (5, 20000, 16, 1025), (5, 16400, 16, 1024),
                                          (5, 20000, 16, 1280), (5, 1 << 31, 16, 500), (5, 20000, 513, 500),
                                          (5, 20000, 0, 500), (0, 20000, 16, 500), (5, 20000, 16, 0)])
def test_workspace_size_is_zero_for_what_the_fused_search_does_not_serve(rows, n, dim, k):
    from recbox_amd import _lib
    assert k > 1024 or k <= 0 or dim > 512 or dim < 1 or rows == 0 or n >= 1 << 31 or sample_rank(n, k) == 0
    assert _lib.lib.rbx_search_ip_workspace_size(rows, n, dim, k) == 0
    if rows > 0 and k > 0:
        rc = _lib.lib.rbx_search_ip(FAKE, rows, max(dim, 1), FAKE, n, dim, k, FAKE, FAKE, FAKE, FAKE, 1 << 40, None)
        assert rc == _lib.RBX_ERR_UNSUPPORTED
        assert "search_ip" in _lib.last_error()


@pytest.mark.parametrize("rows,n,dim,k", [(5, 20000, 16, 500), (1, 16500, 1, 1024), (1000, 10 ** 7, 128, 500),
                                          (70, 70001, 512, 1)])
def test_workspace_size_is_positive_where_the_rank_rule_is_selective(rows, n, dim, k):
    from recbox_amd import _lib
    assert sample_rank(n, k) > 0
    size = _lib.lib.rbx_search_ip_workspace_size(rows, n, dim, k)
    # thr / cnt / fail words per row + 8 192 candidate slots of (int64 item, fp32 score) per row
    assert size >= rows * (12 + 8192 * 12)
    assert size <= rows * (12 + 8192 * 12) + 4096


def test_refused_arguments_never_reach_the_device():
    from recbox_amd import _lib
    lib = _lib.lib
    assert lib.rbx_search_ip(None, 5, 16, FAKE, 20000, 16, 500, FAKE, FAKE, FAKE, FAKE, 1 << 40, None) == _lib.RBX_ERR_INVALID
    assert lib.rbx_search_ip(FAKE, 5, 8, FAKE, 20000, 16, 500, FAKE, FAKE, FAKE, FAKE, 1 << 40, None) == _lib.RBX_ERR_INVALID
    assert lib.rbx_search_ip(FAKE, 5, 16, FAKE, 20000, 16, 500, FAKE, FAKE, FAKE, FAKE, 16, None) == _lib.RBX_ERR_WORKSPACE
    assert lib.rbx_search_ip(FAKE, 0, 16, FAKE, 20000, 16, 500, FAKE, FAKE, FAKE, None, 0, None) == _lib.RBX_OK


def test_search_ip_raises_on_cpu_tensors():
    from recbox_amd import ops
    with pytest.raises(RuntimeError, match="GPU"):
        ops.search_ip(torch.zeros(2, 4), torch.zeros(20000, 4), 5)
    assert set(ops.search_ip_stats) == {"fused_rows", "fallback_rows"}
