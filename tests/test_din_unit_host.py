"""DIN's activation unit (csrc/rbx_din.hip), the parts that need no GPU: the C ABI's five entry points are declared,
exported and bound; the version stays put; the backward's workspace grows with the batch; the rechub mirrors are in the
compat table; the ops refuse CPU tensors."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["rbx_din_pairs_fwd", "rbx_din_pairs_bwd_workspace_size", "rbx_din_pairs_bwd", "rbx_din_pool_fwd", "rbx_din_pool_bwd"]


def _header():
    with open(os.path.join(ROOT, "include", "recbox_hip.h")) as fh:
        return fh.read()


def test_header_declares_the_entry_points_and_keeps_the_version():
    text = _header()
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


def test_workspace_size_is_finite_and_monotone_in_batch():
    from recbox_amd import _lib
    size = _lib.lib.rbx_din_pairs_bwd_workspace_size
    last = 0
    for batch in (1, 2, 37, 100, 4096, 100000):
        now = size(batch, 50, 64, 36)
        assert 0 < now < (1 << 34), (batch, now)
        assert now >= last
        last = now
    assert size(4096, 50, 64, 36) > size(1, 50, 64, 36)
    # one partial [n, 4 dim] + [n] per split of the row range, whatever the batch
    assert size(1, 1, 4, 1) >= (1 * 16 + 1) * 4
    assert size(0, 50, 64, 36) == 0


def test_shape_refusals_need_no_gpu():
    """The shape checks come before anything touches the device: E = 6, E = 132, n = 65 -> RBX_ERR_UNSUPPORTED."""
    from recbox_amd import _lib
    for dim, n in ((6, 8), (132, 8), (64, 65), (64, 0)):
        rc = _lib.lib.rbx_din_pairs_fwd(None, 0, None, 0, 4, 5, dim, None, None, n, 0, None, None)
        assert rc == _lib.RBX_ERR_UNSUPPORTED, (dim, n, rc)
        assert _lib.last_error()
    assert _lib.lib.rbx_din_pool_fwd(None, None, None, 0, 4, 5, 6, 1, None, None, None) == _lib.RBX_ERR_UNSUPPORTED
    assert _lib.lib.rbx_din_pool_bwd(None, None, None, None, 0, 4, 5000, 8, 1, None, None, None) == _lib.RBX_ERR_UNSUPPORTED
    assert _lib.lib.rbx_din_pairs_fwd(None, 0, None, 0, 0, 5, 8, None, None, 4, 0, None, None) == _lib.RBX_OK   # batch = 0


def test_compat_table_names_the_rechub_mirrors():
    from recbox_amd import compat
    table = compat.alias_table()
    for root in ("torch_rechub", "recbox.third_party.rechub"):
        target, names = table[root + ".models.ranking.din"]
        assert target == "recbox_amd.rechub.models.ranking" and {"DIN", "ActivationUnit"} <= set(names)
        assert "DIN" in table[root + ".models.ranking"][1]
    from recbox_amd.rechub.models import ranking
    assert ranking.DIN.__module__ == ranking.ActivationUnit.__module__ == "recbox_amd.rechub.models.ranking"


def test_ops_refuse_cpu_tensors():
    from recbox_amd import ops
    h, t, w = torch.randn(3, 5, 8), torch.randn(3, 8), torch.randn(4, 32)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.din_scores(h, t, w)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.din_pool(torch.randn(3, 5), h)


def test_switches_default_to_fused_from_width_32_up():
    """din_fused / din_min_dim are what the environment said at import, and on / 32 where it said nothing."""
    from recbox_amd import ops
    assert ops.config.din_fused is (os.environ.get("RECBOX_AMD_DIN_FUSED", "1") != "0")
    assert ops.config.din_min_dim == int(os.environ.get("RECBOX_AMD_DIN_MIN_DIM", "32"))
