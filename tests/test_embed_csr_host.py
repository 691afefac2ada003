"""CPU-only checks of the ragged (CSR) multi-hot lookup's surface: include/recbox_hip.h declares rbx_bag_t and the four
rbx_embed_csr_* entry points, the built library exports them, recbox_amd._lib binds them with a struct of the C layout, and
the host layer has ops.Bags / ops.embed_bags / ops.bags_from_padded, which refuse CPU tensors like every op.  The kernels
themselves are tested on the GPU: tests/test_gpu_embed_csr.py."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

from conftest import ROOT

ENTRY_POINTS = ("rbx_embed_csr_fwd", "rbx_embed_csr_bwd_workspace_size", "rbx_embed_csr_sort", "rbx_embed_csr_bwd")


def _header():
    return open(os.path.join(ROOT, "include", "recbox_hip.h")).read()


def test_header_declares_the_bag_descriptor_and_the_four_entry_points():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"typedef\s+struct\s+rbx_bag\s*\{[^}]*\}\s*rbx_bag_t\s*;", text)
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(\s*const\s+rbx_bag_t\s*\*" % name, text), "%s(const rbx_bag_t* ...) is not declared" % name
    assert re.search(r"#define\s+RBX_VERSION\s+124\b", text)               # additions only: the number stays


def test_library_exports_and_lib_binds_the_entry_points():
    from recbox_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert hasattr(raw, name), "librecbox_hip.so does not export %s" % name
        assert name in _lib.SIGNATURES
        assert getattr(_lib.lib, name).argtypes[0] is ctypes.POINTER(_lib.rbx_bag_t)
    assert _lib.lib.rbx_embed_csr_bwd_workspace_size.restype is ctypes.c_size_t
    m = re.search(r"#define\s+RBX_MAX_BAGS\s+(\d+)", _header())
    assert m and int(m.group(1)) == _lib.RBX_MAX_BAGS


def test_bag_struct_has_the_c_layout(tmp_path):
    """sizeof and every member's offset, from a probe compiled against the header with the host compiler."""
    from recbox_amd import _lib
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no host C compiler to probe the layout of rbx_bag_t with")
    names = [n for n, _ in _lib.rbx_bag_t._fields_]
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "recbox_hip.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(rbx_bag_t));\n'
                   + "".join('  printf(" %%zu", offsetof(rbx_bag_t, %s));\n' % n for n in names)
                   + "  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.run([cc, "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout.split()]
    assert ctypes.sizeof(_lib.rbx_bag_t) == got[0] == 104
    assert [getattr(_lib.rbx_bag_t, n).offset for n in names] == got[1:]
    members = re.search(r"typedef\s+struct\s+rbx_bag\s*\{(.*?)\}\s*rbx_bag_t", _header(), flags=re.S).group(1)
    declared = re.findall(r"(\w+)\s*;", re.sub(r"/\*.*?\*/", "", members, flags=re.S))
    assert declared == names                                               # same members, same order


def test_host_surface_exists():
    from recbox_amd import ops
    for name in ("Bags", "embed_bags", "bags_from_padded", "BagSpec", "BagPlan"):
        assert hasattr(ops, name), "recbox_amd.ops.%s is missing" % name


def test_bags_and_embed_bags_refuse_cpu_tensors():
    """No CPU fallback: the carrier, the converter and the op raise on CPU tensors."""
    from recbox_amd import _lib, ops
    idx, off = torch.tensor([1, 2, 3]), torch.tensor([0, 1, 3])
    with pytest.raises(RuntimeError, match="GPU"):
        ops.Bags(idx, off)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.bags_from_padded(torch.zeros(2, 3, dtype=torch.long), 0)
    bags = ops.Bags.__new__(ops.Bags)                                      # a carrier built around the checks
    bags.indices, bags.offsets = idx, off
    w = torch.nn.Parameter(torch.zeros(5, 4))
    spec = ops.BagSpec("hist", 4, 0, 0, _lib.POOL_SUM, 5)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.embed_bags([spec], [bags], [w])
    with pytest.raises(TypeError):
        ops.embed_bags([spec], [idx], [w])


def test_pools_that_keep_one_slot_per_id_are_refused_by_the_plan():
    from recbox_amd import _lib, ops
    for pool in (_lib.POOL_NONE, _lib.POOL_CONCAT):
        with pytest.raises(NotImplementedError):
            ops.BagPlan([ops.BagSpec("hist", 4, 0, 0, pool, 5)])
