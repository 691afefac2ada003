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


# ---- the refusals of the walk drivers and the position-valued reduces: return code and message, before any device call ----
FAKE = 0x10000                                             # a non-NULL "device pointer" no refused call may touch


def _bag(pool, nnz=5000, dim=8, grad=True):
    from recbox_amd import _lib
    b = _lib.rbx_bag_t()
    b.indices, b.offsets, b.table, b.grad = FAKE, FAKE, FAKE, (FAKE if grad else None)
    b.nnz, b.indices_stride, b.vocab = nnz, 1, 50
    b.padding_idx, b.mask_id, b.out_off = _lib.RBX_NO_ID, _lib.RBX_NO_ID, 0
    b.dim, b.indices_dtype, b.offsets_dtype, b.pool, b.eps, b.reserved = dim, _lib.RBX_I64, _lib.RBX_I64, pool, 0.0, 0
    return b


def _refusal_cases():
    """(label, call, return code, message or None).  Every call here ends before a memset or a launch: it is refused, or
    it has no bag to walk and returns in front of its first device call."""
    from recbox_amd import _lib
    lib, OK, I, U, W = _lib.lib, _lib.RBX_OK, _lib.RBX_ERR_INVALID, _lib.RBX_ERR_UNSUPPORTED, _lib.RBX_ERR_WORKSPACE
    one = lambda b: (_lib.rbx_bag_t * 1)(b)
    total, mean, peak = one(_bag(_lib.POOL_SUM)), one(_bag(_lib.POOL_MEAN_ID)), one(_bag(_lib.POOL_MAX))
    frozen_mean = (_lib.rbx_bag_t * 2)(_bag(_lib.POOL_SUM), _bag(_lib.POOL_MEAN_ID, grad=False))
    w, w2, T, B = (ctypes.c_void_p * 1)(FAKE), (ctypes.c_void_p * 2)(None, FAKE), 64, 4
    lneed = lib.rbx_embed_csr_fwd_long_workspace_size(total, 1, B, T)
    mneed = lib.rbx_embed_csr_fwd_max_workspace_size(peak, 1, B, T)
    bneed = lib.rbx_embed_csr_bwd_workspace_size(total, 1, B)
    assert 256 < lneed < mneed and bneed > 0
    short = lambda have, need: "workspace %d B < required %d B" % (have, need)
    fwd = lambda bags, batch=B, out=FAKE: lib.rbx_embed_csr_fwd(bags, 1, batch, out, 8, None, None, None)
    fwd_long = lambda bags, batch=B, out=FAKE, ws=FAKE, n=lneed: lib.rbx_embed_csr_fwd_long(
        bags, 1, batch, T, out, 8, None, ws, n, None, None)
    fwd_wl = lambda bags, batch=B, out=FAKE, ws=FAKE, n=lneed: lib.rbx_embed_csr_fwd_weighted_long(
        bags, 1, batch, T, w, out, 8, ws, n, None, None)
    wg_long = lambda bags, batch=B, dout=FAKE, dw=w, ws=FAKE, n=lneed: lib.rbx_embed_csr_weight_grad_long(
        bags, 1, batch, T, dout, 8, dw, ws, n, None, None)
    fwd_max = lambda bags, batch=B, out=FAKE, arg=FAKE, ws=FAKE, n=mneed, t=T: lib.rbx_embed_csr_fwd_max(
        bags, 1, batch, t, out, 8, arg, 8, ws, n, None, None)
    bwd_w = lambda bags, batch=B, dout=FAKE, ws=FAKE, n=bneed, nb=1, wt=w: lib.rbx_embed_csr_bwd_weighted(
        bags, nb, batch, wt, dout, 8, 0, ws, n, None)
    bwd_max = lambda bags, batch=B, dout=FAKE, arg=FAKE, ws=FAKE, n=bneed, astride=8: lib.rbx_embed_csr_bwd_max(
        bags, 1, batch, dout, 8, arg, astride, 0, ws, n, None)
    wide = one(_bag(_lib.POOL_MAX, dim=1024))
    return [
        ("fwd: NULL d_out", lambda: fwd(total, out=None), I, "d_out is NULL"),
        ("fwd: max pool", lambda: fwd(peak), U, "the sum / mean forward: bag 0 is a max pool"),
        ("fwd: batch 0", lambda: fwd(total, 0, None), OK, None),
        ("fwd_long: NULL d_out", lambda: fwd_long(total, out=None), I, "d_out is NULL"),
        ("fwd_long: max pool", lambda: fwd_long(peak), U, "the sum / mean forward: bag 0 is a max pool"),
        ("fwd_long: no workspace", lambda: fwd_long(total, ws=None, n=0), W, short(0, lneed)),
        ("fwd_long: NULL workspace of a size", lambda: fwd_long(total, ws=None), W, short(0, lneed)),
        ("fwd_long: small workspace", lambda: fwd_long(total, n=lneed - 1), W, short(lneed - 1, lneed)),
        ("fwd_long: batch 0, no workspace", lambda: fwd_long(total, 0, None, None, 0), W, short(0, 256)),   # the header is cleared
        ("fwd_weighted_long: NULL d_out", lambda: fwd_wl(total, out=None), I, "d_out is NULL"),
        ("fwd_weighted_long: max pool", lambda: fwd_wl(peak), U, "the sum / mean forward: bag 0 is a max pool"),
        ("fwd_weighted_long: weights on a mean pool", lambda: fwd_wl(mean), U, "bag 0: a weight array with pool mode 3"),
        ("fwd_weighted_long: no workspace", lambda: fwd_wl(total, ws=None, n=0), W, short(0, lneed)),
        ("fwd_weighted_long: small workspace", lambda: fwd_wl(total, n=lneed - 1), W, short(lneed - 1, lneed)),
        ("fwd_weighted_long: batch 0, no workspace", lambda: fwd_wl(total, 0, None, None, 0), W, short(0, 256)),
        ("weight_grad_long: NULL d_dout", lambda: wg_long(total, dout=None), I, "d_dout is NULL"),
        ("weight_grad_long: NULL d_dweights", lambda: wg_long(total, dw=None), I, "d_dweights is NULL"),
        ("weight_grad_long: max pool", lambda: wg_long(peak), U, "the weight gradient: bag 0 is a max pool"),
        ("weight_grad_long: mean pool", lambda: wg_long(mean), U, "bag 0: a weight gradient with pool mode 3"),
        ("weight_grad_long: no workspace", lambda: wg_long(total, ws=None, n=0), W, short(0, lneed)),
        ("weight_grad_long: small workspace", lambda: wg_long(total, n=lneed - 1), W, short(lneed - 1, lneed)),
        ("weight_grad_long: batch 0, no workspace", lambda: wg_long(total, 0, None, w, None, 0), W, short(0, 256)),
        ("fwd_max: NULL d_out", lambda: fwd_max(peak, out=None), I, "d_out is NULL"),
        ("fwd_max: NULL d_argpos", lambda: fwd_max(peak, arg=None), I, "d_argpos is NULL"),
        ("fwd_max: sum pool", lambda: fwd_max(total), U, "rbx_embed_csr_fwd_max: bag 0 has pool mode 1"),
        ("fwd_max: no workspace", lambda: fwd_max(peak, ws=None, n=0), W, short(0, mneed)),
        ("fwd_max: the long workspace is too small", lambda: fwd_max(peak, n=lneed), W, short(lneed, mneed)),
        ("fwd_max: batch 0, no workspace", lambda: fwd_max(peak, 0, None, None, None, 0), OK, None),
        ("fwd_max: batch 0, with a workspace", lambda: fwd_max(peak, 0), OK, None),
        ("fwd_max: batch 0, threshold 0, no workspace", lambda: fwd_max(peak, 0, None, None, None, 0, 0), OK, None),
        ("fwd_max: negative threshold", lambda: fwd_max(peak, 0, t=-1), I, "negative long_threshold"),
        ("bwd_weighted: NULL d_dout", lambda: bwd_w(total, dout=None), I, "d_dout is NULL"),
        ("bwd_weighted: max pool", lambda: bwd_w(peak), U, "rbx_embed_csr_bwd_weighted: bag 0 is a max pool"),
        ("bwd_weighted: trained mean pool", lambda: bwd_w(mean), U, "rbx_embed_csr_bwd_weighted: bag 0 is a mean pool with a gradient"),
        ("bwd_weighted: weights on a frozen mean pool", lambda: bwd_w(frozen_mean, nb=2, wt=w2), U,
         "bag 1: a weight array with pool mode 3"),
        ("bwd_weighted: no workspace", lambda: bwd_w(total, ws=None, n=0), W, short(0, bneed)),
        ("bwd_weighted: small workspace", lambda: bwd_w(total, n=bneed - 1), W, short(bneed - 1, bneed)),
        ("bwd_weighted: batch 0, no workspace", lambda: bwd_w(total, 0, ws=None, n=0), OK, None),
        ("bwd_weighted: batch 0, with a workspace", lambda: bwd_w(total, 0), OK, None),
        ("bwd_max: NULL d_dout", lambda: bwd_max(peak, dout=None), I, "d_dout is NULL"),
        ("bwd_max: NULL d_argpos", lambda: bwd_max(peak, arg=None), I, "d_argpos is NULL"),
        ("bwd_max: sum pool", lambda: bwd_max(total), U, "rbx_embed_csr_bwd_max: bag 0 has pool mode 1"),
        ("bwd_max: no workspace", lambda: bwd_max(peak, ws=None, n=0), W, short(0, bneed)),
        ("bwd_max: small workspace", lambda: bwd_max(peak, n=bneed - 1), W, short(bneed - 1, bneed)),
        ("bwd_max: batch 0, no workspace", lambda: bwd_max(peak, 0, ws=None, n=0), OK, None),
        ("bwd_max: batch 0, with a workspace", lambda: bwd_max(peak, 0), OK, None),
        ("bwd_max: scalar argpos rows at dim 1024", lambda: bwd_max(wide, n=1 << 30, astride=1026), U,
         "embedding dim 1024 too large for one lane group (scalar units: d_argpos is not 16-byte aligned"),
    ]


def test_walk_drivers_and_position_reduces_refuse_with_their_code_and_message():
    from recbox_amd import _lib
    for label, call, code, message in _refusal_cases():
        assert call() == code, "%s: %s" % (label, _lib.last_error())
        if message is not None:
            assert message in _lib.last_error(), "%s: %r" % (label, _lib.last_error())
