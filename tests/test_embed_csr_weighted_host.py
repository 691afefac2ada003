"""CPU-only checks of the per-sample weights of the ragged (CSR) lookup: include/recbox_hip.h declares the weighted entry
points next to the four unweighted ones, the built library exports them, recbox_amd._lib binds them; RBX_VERSION and the
layout of rbx_bag_t did not move (the weights travel beside the descriptors); ops.Bags takes the weights, refuses what is
not a float32 [nnz] tensor on the GPU, and a weighted bag on a mean pool is refused when the plan is bound.  The kernels
are tested on the GPU: tests/test_gpu_embed_csr_weighted.py."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from conftest import ROOT

ENTRY_POINTS = ("rbx_embed_csr_fwd_weighted", "rbx_embed_csr_sort_weighted", "rbx_embed_csr_bwd_weighted",
                "rbx_embed_csr_weight_grad")


def _header():
    return open(os.path.join(ROOT, "include", "recbox_hip.h")).read()


def test_header_declares_the_weighted_entry_points_and_keeps_version_and_descriptor():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(\s*const\s+rbx_bag_t\s*\*" % name, text), "%s(const rbx_bag_t* ...) is not declared" % name
    assert re.search(r"rbx_embed_csr_fwd_weighted\s*\([^)]*const\s+float\s*\*\s*const\s*\*\s*d_weights", text)
    assert re.search(r"rbx_embed_csr_bwd_weighted\s*\([^)]*const\s+float\s*\*\s*const\s*\*\s*d_weights", text)
    assert re.search(r"rbx_embed_csr_weight_grad\s*\([^)]*float\s*\*\s*const\s*\*\s*d_dweights", text)
    assert re.search(r"#define\s+RBX_VERSION\s+124\b", text)
    for name in ENTRY_POINTS:                                              # documented in the block above rbx_bag_t
        block = _header()[:_header().index("typedef struct rbx_bag")]
        assert name in block, "%s is not described in the header's comment" % name


def test_library_exports_and_lib_binds_the_weighted_entry_points():
    from recbox_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert hasattr(raw, name), "librecbox_hip.so does not export %s" % name
        assert name in _lib.SIGNATURES
        assert getattr(_lib.lib, name).argtypes[0] is ctypes.POINTER(_lib.rbx_bag_t)
    assert _lib.lib.rbx_version() == 124
    assert ctypes.sizeof(_lib.rbx_bag_t) == 104
    assert [n for n, _ in _lib.rbx_bag_t._fields_] == ["indices", "offsets", "table", "grad", "nnz", "indices_stride", "vocab",
                                                       "padding_idx", "mask_id", "out_off", "dim", "indices_dtype",
                                                       "offsets_dtype", "pool", "eps", "reserved"]


def test_bags_takes_weights_as_third_argument():
    from recbox_amd import ops
    assert list(inspect.signature(ops.Bags.__init__).parameters)[1:4] == ["indices", "offsets", "weights"]
    assert inspect.signature(ops.Bags.__init__).parameters["weights"].default is None
    assert list(inspect.signature(ops.bags_from_padded).parameters) == ["ids", "mask_id", "weights"]


def test_weighted_bags_and_embed_bags_refuse_cpu_tensors():
    from recbox_amd import _lib, ops
    idx, off, w = torch.tensor([1, 2, 3]), torch.tensor([0, 1, 3]), torch.ones(3)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.Bags(idx, off, w)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.bags_from_padded(torch.zeros(2, 3, dtype=torch.long), 0, torch.ones(2, 3))
    bags = ops.Bags.__new__(ops.Bags)                                      # a carrier built around the checks
    bags.indices, bags.offsets, bags.weights = idx, off, w
    table = torch.nn.Parameter(torch.zeros(5, 4))
    spec = ops.BagSpec("hist", 4, 0, 0, _lib.POOL_SUM, 5)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.embed_bags([spec], [bags], [table])


@pytest.mark.parametrize("pool", ["POOL_MEAN_ID", "POOL_MEAN_VALUE"])
def test_weighted_bag_on_a_mean_spec_is_refused_when_the_plan_is_bound(pool):
    """Without a GPU: the plan looks at the carrier before it takes any pointer."""
    from recbox_amd import _lib, ops
    bags = ops.Bags.__new__(ops.Bags)
    bags.indices, bags.offsets, bags.weights = torch.tensor([1, 2, 3]), torch.tensor([0, 1, 3]), torch.ones(3)
    plan = ops.BagPlan([ops.BagSpec("dwell", 4, 0, 0, getattr(_lib, pool), 5, eps=1e-8)])
    with pytest.raises(NotImplementedError, match="dwell"):
        plan.bind_inputs([bags])
