"""The field-aware FM kernels (csrc/rbx_ffm.hip: ffm_fwd_kernel<D4C, REDUCE>, FfmPolicy over the sorted segmented reduce) at
every form the launcher dispatches, against the restatement of tests/ffm64.py under the scale-aware bar of tests/fp32_bar.py:
per tensor max|got - want| <= max(4 e32, 2e-6 max|want|), e32 the error of the same restatement run in float32 on the CPU
(ffm64.manual: the gathers, one multiply per element, index_add_ in the order of the samples; tests/test_fp32_bar_host.py holds
it to autograd over ffm64.cross).  Nothing the kernels return enters the bar; the factor is 4 everywhere.  The Hadamard forward
is one fp32 multiply per element and is compared bit for bit with ffm64.cross in fp32.  Upstream gradients are at unit scale:
tests/test_gpu_ffm.py scales them by 1 / sqrt(B) in its multiplicity test to fit the absolute 1e-4.

Forms:
  D = 4, 8, 16, 32 (D4C = 1, 2, 4, 8) and 12, 20, 64, 128 (the generic form), each at F = 5, B = 37 and at F = 2, B = 1, both
  reduce forms; F = 3 at B = 65 (21 samples per wavefront task: 4 tasks, the last with 2 samples); F = 33 (one sample per task,
  31 lanes idle in the id fetch) and F = 64 (every lane fetches an id).
  The grid-stride loop: the grid is capped at kCUs * 8 = 2048 workgroups of 4 wavefronts, so 8192 wavefronts; at F = 33 a task
  is one sample, and B = 8200 gives the first 8 wavefronts a second trip.  D = 4 and vocabularies of 1 .. 3 blocks keep the
  float64 restatement at 2 s (measured on the CPU).
  Multiplicity at unit gradient: vocabularies of 1 and 3 blocks at B = 6181 -- runs of thousands of equal keys through the
  reduce's chunk summaries; e32 grows with the run (the float32 restatement adds the samples one after another).
  Small tables and gradients (ffm64.small_mult_case, small_wide_case: the inputs of the host test's mutants).
  Through the C ABI: out_stride_b / dout_stride_b wider than the row, NaN guards between the rows and around every output, and
  the backward's accumulate form (rbx_ffm_bwd's ``accumulate`` argument) onto a prefilled gradient.
A spy on ops.lib counts rbx_ffm_fwd / rbx_ffm_bwd: the kernels ran, not the F.embedding composition of the models.

Measured on the MI355X, worst err / bar over all cases of this module (38 tests, 5.7 s): out 0.20 (D = 128, summed), dtable
0.09; multiplicity at B = 6181 and unit gradient: dtable 0.055 -- the segmented reduce is closer to float64 than adding the
samples one after another in fp32 is.  Every kernel holds the bar with the factor 4; nothing had to be fixed.
Mutation check (a scratch build, never committed): ffm_fwd_kernel's task loop ended after a wavefront's first task
(``task < n_tasks && task < n_waves``) leaves the last 8 samples of B = 8200 unwritten: both cases of
test_second_trip_of_the_grid_stride_loop fail, all 62 tests of tests/test_gpu_ffm.py pass."""
import os
import re

import pytest
import torch

import ffm64
from fp32_bar import assert_bar, report
from guarded import Guarded, ptr as _p

pytestmark = pytest.mark.gpu
B = 37
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _spy(monkeypatch):
    from recbox_amd import ops
    calls = []
    real = ops.lib

    class Spy(object):
        def rbx_ffm_fwd(self, *a):
            calls.append("fwd")
            return real.rbx_ffm_fwd(*a)

        def rbx_ffm_bwd(self, *a):
            calls.append("bwd")
            return real.rbx_ffm_bwd(*a)

        def __getattr__(self, name):
            return getattr(real, name)
    monkeypatch.setattr(ops, "lib", Spy())
    return calls


def _fused(case, reduce_sum):
    from recbox_amd import ops
    ts = [t.cuda().requires_grad_(True) for t in case["tables"]]
    out = ops.ffm_cross(ts, [x.cuda() for x in case["ids"]], reduce_sum=reduce_sum)
    grads = torch.autograd.grad(out, ts, case["r"][bool(reduce_sum)].cuda())
    return out.detach(), list(grads)


def _check(case, reduce_sum, tag, exact_forward=True):
    """Runs the op on ``case`` and holds out and every dtable to the bar; the Hadamard forward to the bits of fp32."""
    want, ref32 = ffm64.manual(case, reduce_sum), ffm64.manual(case, reduce_sum, torch.float32)
    out, grads = _fused(case, reduce_sum)
    if not reduce_sum and exact_forward:
        assert torch.equal(out.cpu(), ffm64.cross(case["tables"], case["ids"])), tag
    assert_bar("out %s" % tag, out, want[0], ref32[0])
    for i, g in enumerate(grads):
        assert_bar("dtable %s table %d" % (tag, i), g, want[1][i], ref32[1][i])
    return out, grads


@pytest.mark.parametrize("reduce_sum", [False, True])
@pytest.mark.parametrize("D", [4, 8, 16, 32, 12, 20, 64, 128])
def test_every_width_specialisation_and_the_generic_form(D, reduce_sum, monkeypatch):
    calls = _spy(monkeypatch)
    _check(ffm64.make_case(5, D, B, seed=1), reduce_sum, "F=5 D=%d B=%d sum=%d" % (D, B, reduce_sum))
    _check(ffm64.make_case(2, D, 1, seed=2), reduce_sum, "F=2 D=%d B=1 sum=%d" % (D, reduce_sum))
    assert calls == ["fwd", "bwd"] * 2
    report("ffm D=%d sum=%d" % (D, reduce_sum))


@pytest.mark.parametrize("reduce_sum", [False, True])
@pytest.mark.parametrize("F,D,batch", [(3, 16, 65), (33, 8, B), (64, 16, B), (33, 28, 3)])
def test_samples_per_wavefront_task(F, D, batch, reduce_sum, monkeypatch):
    calls = _spy(monkeypatch)
    _check(ffm64.make_case(F, D, batch, seed=3), reduce_sum, "F=%d D=%d B=%d sum=%d" % (F, D, batch, reduce_sum))
    assert calls == ["fwd", "bwd"]
    report("ffm F=%d D=%d sum=%d" % (F, D, reduce_sum))


@pytest.mark.parametrize("reduce_sum", [False, True])
def test_second_trip_of_the_grid_stride_loop(reduce_sum, monkeypatch):
    with open(os.path.join(ROOT, "recbox_amd", "csrc", "rbx_internal.h")) as fh:
        k_cus = int(re.search(r"constexpr int kCUs = (\d+);", fh.read()).group(1))
    F, D = 33, 4
    waves = k_cus * 8 * 4                                     # the capped grid: kCUs * 8 workgroups of 4 wavefronts
    batch = waves + 8                                         # one sample per task at F = 33: 8 wavefronts go round again
    assert (k_cus, batch) == (256, 8200) and 64 // F == 1
    calls = _spy(monkeypatch)
    case = ffm64.make_case(F, D, batch, seed=3, blocks=[1 + i % 3 for i in range(F)])
    out, _ = _check(case, reduce_sum, "second trip F=33 D=4 B=%d sum=%d" % (batch, reduce_sum))
    assert calls == ["fwd", "bwd"]
    # the samples of the second trip on their own
    want = ffm64.cross([t.double() for t in case["tables"]], [x[waves:] for x in case["ids"]], reduce_sum)
    ref32 = ffm64.cross(case["tables"], [x[waves:] for x in case["ids"]], reduce_sum)
    assert_bar("out[second trip] sum=%d" % reduce_sum, out[waves:], want, ref32)
    report("ffm second trip sum=%d" % reduce_sum)


@pytest.mark.parametrize("reduce_sum", [False, True])
@pytest.mark.parametrize("batch", [6181, 1])
def test_multiplicity_at_unit_gradient(batch, reduce_sum, monkeypatch):
    calls = _spy(monkeypatch)
    case = ffm64.make_case(5, 16, batch, seed=2, blocks=[1, 3, 1, 3, 3])
    _check(case, reduce_sum, "multiplicity B=%d sum=%d" % (batch, reduce_sum))
    assert calls == ["fwd", "bwd"]
    report("ffm multiplicity B=%d sum=%d" % (batch, reduce_sum))


@pytest.mark.parametrize("reduce_sum", [False, True])
def test_small_tables_and_small_upstream_gradient(reduce_sum, monkeypatch):
    """Tables at std 1e-3, upstream at 1e-3: every gradient is below 2e-4, the summed forward below 4e-5."""
    calls = _spy(monkeypatch)
    _check(ffm64.small_mult_case(), reduce_sum, "small multiplicity sum=%d" % reduce_sum)
    _check(ffm64.small_wide_case(), reduce_sum, "small D=128 sum=%d" % reduce_sum)
    assert calls == ["fwd", "bwd"] * 2
    report("ffm small sum=%d" % reduce_sum)


@pytest.mark.parametrize("reduce_sum", [False, True])
@pytest.mark.parametrize("F,D,batch", [(5, 16, B), (3, 12, 65), (33, 4, B)])
def test_c_abi_strided_rows_guards_and_the_accumulate_form(F, D, batch, reduce_sum):
    from recbox_amd import _lib, ops
    lib = _lib.lib
    case = ffm64.make_case(F, D, batch, seed=4)
    P = F * (F - 1) // 2
    width = P if reduce_sum else P * D
    pad = 12                                                   # (a multiple of 4: the Hadamard rows stay float4-addressable)
    tables = [t.cuda() for t in case["tables"]]
    ids = [x.cuda() for x in case["ids"]]
    plan = ops._ffm_plan(F, D, [t.shape[0] for t in tables])
    _, keep = plan.bind_inputs(ids)
    plan.bind_params(tables)
    out = Guarded(batch, width, stride=width + pad)
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    rc = lib.rbx_ffm_fwd(plan.arr, F, batch, int(reduce_sum), _p(out.view), width + pad, _p(status), None)
    assert rc == _lib.RBX_OK, _lib.last_error()
    torch.cuda.synchronize()
    assert int(status) == 0 and out.untouched()
    want, ref32 = ffm64.manual(case, reduce_sum), ffm64.manual(case, reduce_sum, torch.float32)
    tag = "c-abi F=%d D=%d B=%d sum=%d" % (F, D, batch, reduce_sum)
    if not reduce_sum:
        assert torch.equal(out.view.cpu().reshape(batch, P, D), ffm64.cross(case["tables"], case["ids"]))
    assert_bar("out " + tag, out.view.reshape(want[0].shape), want[0], ref32[0])

    dout = Guarded(batch, width, stride=width + pad, fill=case["r"][bool(reduce_sum)])
    g = torch.Generator().manual_seed(5)
    prefill = [torch.randn(t.shape, generator=g) for t in case["tables"]]
    for accumulate in (0, 1):
        grads = [Guarded(t.shape[0], D, fill=(pf if accumulate else 0.0)) for t, pf in zip(tables, prefill)]
        plan.bind_params(tables, [gr.view for gr in grads])
        ws_bytes = lib.rbx_ffm_bwd_workspace_size(plan.arr, F, batch)
        assert ws_bytes > 0
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
        rc = lib.rbx_ffm_sort(plan.arr, F, batch, _p(ws), ws_bytes, None, None)
        assert rc == _lib.RBX_OK, _lib.last_error()
        rc = lib.rbx_ffm_bwd(plan.arr, F, batch, int(reduce_sum), _p(dout.view), width + pad, accumulate, _p(ws), ws_bytes, None)
        assert rc == _lib.RBX_OK, _lib.last_error()
        torch.cuda.synchronize()
        for i, gr in enumerate(grads):
            assert gr.untouched(), "dtable %d: a guard band was written" % i
            if accumulate:
                w64, r32 = prefill[i].double() + want[1][i], prefill[i] + ref32[1][i]
            else:
                w64, r32 = want[1][i], ref32[1][i]
            assert_bar("dtable %s accumulate=%d table %d" % (tag, accumulate, i), gr.view, w64, r32)
        assert dout.untouched()
    del keep
    report("ffm " + tag)
