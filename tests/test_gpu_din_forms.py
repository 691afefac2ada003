"""DIN's activation unit kernels (csrc/rbx_din.hip) at every form their launchers dispatch, through the C ABI, against the
restatement of tests/din64.py under the scale-aware bar of tests/fp32_bar.py: per tensor max|got - want| <= max(4 e32,
2e-6 max|want|), e32 the error of the same restatement run in float32 on the CPU.  Nothing the kernels return enters the bar;
the factor is 4 everywhere.  Upstream gradients are at unit scale (tests/test_gpu_din_unit.py scales them by 1 / sqrt(L) to fit
its absolute 1e-4), plus one case per op at 1e-3.

Every output is a view into a NaN-filled buffer with 64 floats of guard on both sides: an element the kernel did not write is
NaN (and fails the bar), a store past the end lands in a guard band, which is asserted untouched.  rc == RBX_OK says the
kernels were launched -- the C ABI has no composition to fall back to.

ReLU: the gate of the backward is the sign of the kernel's own y.  A pre-activation closer to zero than the bar of y may be
gated either way by a correct kernel, so each act = 1 case zeroes the upstream gradient at those elements (a handful, found
on the float64 restatement alone): whichever way the gate falls there, nothing passes through it.

Forms (pairs): 128-row tiles, din_pairs_fwd / din_pairs_dw <1> (n <= 32) and <2>; the dx kernel owns S = 128 / L whole samples:
  (4, 1, 1) the floor; (12, 7, 5) E no multiple of 16 / 32, n odd; (32, 64, 32) S = 2 exactly full; (16, 43, 33) S = 2 with 86
  of 128 rows and B % S = 1, two accumulators; (64, 100, 64) S = 1 with a partly empty tile; (20, 129, 12) one-sample chunks,
  the second of one row; (128, 5, 64) the widest.  M edges of the 1024-row dW splits at E = 8, L = 1, n = 4: M = 1, 1024, 1025
  (a one-row split), 2049 (three splits).  dx with only dhist or only dtarget, dW without db, db without dW: NULLs.
Forms (pool): one workgroup per sample, L walked in strides of 256 (softmax), 8 (forward sum) and 32 (backward dots):
  (1, 4), (8, 128), (255, 12), (256, 16), (257, 16), (4096, 4) at B = 3 = kDinPoolMaxL; 4097 is refused and writes nothing;
  softmax on and off; no mask, a random mask, one sample fully masked (uniform 1 / L under softmax), a mask of {0, 0.5, 1};
  dscore = NULL, dH = NULL.

Measured on the MI355X, worst err / bar over all cases of this module (44 tests, 2.8 s):
  pairs y 0.45, dh 0.17, dt 0.22, dW 0.77 (M = 1024, one full split), db 0.29; pool weight 0.10, out 0.46 (L = 4096),
  dscore 0.30 (the peaked softmax), dh 0.09.  Every kernel holds the bar with the factor 4; nothing had to be fixed.
Mutation check (a scratch build, never committed): din_pool_bwd_kernel selecting on the mask (``if (mask == 0) d = 0``) instead
of multiplying by it fails the five "fractions" cases with L > 1 here and passes all 57 tests of tests/test_gpu_din_unit.py, whose
masks are binary."""
import pytest
import torch

import din64
from fp32_bar import assert_bar, bar_of, report
from guarded import Guarded, ptr as _p, view_of

pytestmark = pytest.mark.gpu
B = 37


def _lib():
    from recbox_amd import _lib as L
    return L


def _run_pairs(case, act, want=("dh", "dt", "dW", "db")):
    """{"y", "dh", "dt", "dW", "db"} through rbx_din_pairs_fwd / _bwd; a gradient not in ``want`` is passed as NULL."""
    L_ = _lib()
    lib = L_.lib
    h, t, w, r = (case[k].cuda() for k in ("h", "t", "w", "r"))
    b = None if case["b"] is None else case["b"].cuda()
    Bn, L, E = h.shape
    n = w.shape[0]
    y = Guarded(Bn * L, n)
    rc = lib.rbx_din_pairs_fwd(_p(h), L * E, _p(t), E, Bn, L, E, _p(w), _p(b), n, act, _p(y.view), None)
    assert rc == L_.RBX_OK, L_.last_error()
    torch.cuda.synchronize()
    out = {"dh": Guarded(Bn * L, E) if "dh" in want else None, "dt": Guarded(Bn, E) if "dt" in want else None,
           "dW": Guarded(n, 4 * E) if "dW" in want else None, "db": Guarded(1, n) if "db" in want else None}
    ws_bytes = lib.rbx_din_pairs_bwd_workspace_size(Bn, L, E, n)
    assert ws_bytes >= ((Bn * L + 1023) // 1024) * (n * 4 * E + n) * 4
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    view = view_of
    rc = lib.rbx_din_pairs_bwd(_p(h), L * E, _p(t), E, Bn, L, E, _p(w), n, act, _p(y.view), _p(r), _p(view(out["dh"])),
                               _p(view(out["dt"])), _p(view(out["dW"])), _p(view(out["db"])), _p(ws), ws_bytes, None)
    assert rc == L_.RBX_OK, L_.last_error()
    torch.cuda.synchronize()
    for name, g in [("y", y)] + list(out.items()):
        assert g is None or g.untouched(), "%s: a guard band was written" % name
    got = {"y": y.view, "dh": out["dh"] and out["dh"].view.view(Bn, L, E), "dt": view(out["dt"]), "dW": view(out["dW"]),
           "db": out["db"] and out["db"].view.view(n)}
    return got


def _pairs_refs(case, act):
    """(want, ref32).  With ReLU the upstream gradient is first zeroed wherever the float64 pre-activation lies within twice
    the bar of y of zero (a handful of elements at most): there a correct kernel may gate either way, and with no gradient
    arriving the choice has no effect.  Decided on the float64 restatement alone."""
    if act:
        pre = din64.pairs_preact(case)
        pre32 = din64.ref_pairs(case["h"], case["t"], case["w"], case["b"], 0)
        bar, _, _ = bar_of(pre, pre32)
        near = pre.abs() <= 2 * bar
        assert int(near.sum()) <= 16
        case["r"][near] = 0.0
    return din64.pairs_reference(case, act), din64.pairs_reference(case, act, torch.float32)


def _assert_pairs(got, want, ref32, tag, names=din64.PAIR_NAMES):
    for n in names:
        if want[n] is None or got.get(n) is None:
            continue
        assert_bar("%s %s" % (n, tag), got[n], want[n], ref32[n])


# E, L, n, bias per act (0, 1)
PAIR_FORMS = [(4, 1, 1, (True, False)), (12, 7, 5, (True, True)), (32, 64, 32, (False, True)), (16, 43, 33, (True, True)),
              (64, 100, 64, (True, False)), (20, 129, 12, (True, True)), (128, 5, 64, (False, True))]


@pytest.mark.parametrize("E,L,n,biases", PAIR_FORMS)
def test_pairs_every_tiling_form(E, L, n, biases):
    for act, bias in enumerate(biases):
        case = din64.pairs_case(E, L, n, bias, 1000 * E + 10 * L + n + act)
        want, ref32 = _pairs_refs(case, act)
        got = _run_pairs(case, act, ("dh", "dt", "dW", "db") if bias else ("dh", "dt", "dW"))
        _assert_pairs(got, want, ref32, "E=%d L=%d n=%d act=%d bias=%d" % (E, L, n, act, bias))
    report("din pairs E=%d L=%d n=%d" % (E, L, n))


@pytest.mark.parametrize("batch", [1, 1024, 1025, 2049])
def test_pairs_row_counts_at_the_edges_of_the_dw_splits(batch):
    E, L, n = 8, 1, 4
    for act in (0, 1):
        case = din64.pairs_case(E, L, n, True, 50 + batch + act, batch=batch)
        want, ref32 = _pairs_refs(case, act)
        got = _run_pairs(case, act)
        _assert_pairs(got, want, ref32, "M=%d act=%d" % (batch, act))
    report("din pairs M=%d" % batch)


@pytest.mark.parametrize("E,L,n", [(12, 7, 5), (16, 43, 33), (20, 129, 12)])
def test_pairs_with_some_gradients_not_wanted(E, L, n):
    case = din64.pairs_case(E, L, n, True, 7 + E)
    want, ref32 = _pairs_refs(case, 1)
    full = _run_pairs(case, 1)
    for names in (("dh",), ("dt",), ("dW",), ("db",), ("dh", "dW"), ("dt", "db")):
        got = _run_pairs(case, 1, names)
        _assert_pairs(got, want, ref32, "E=%d L=%d n=%d only %s" % (E, L, n, "+".join(names)), ("y",) + names)
        for k in names:
            assert torch.equal(got[k], full[k]), k
    report("din pairs NULLs E=%d L=%d n=%d" % (E, L, n))


def test_pairs_small_upstream_gradient():
    """Upstream at 1e-3: every gradient is held to a few 1e-9 instead of 1e-4."""
    for (E, L, n) in ((12, 7, 5), (16, 43, 33)):
        case = din64.pairs_case(E, L, n, True, 5, up=1e-3)
        want, ref32 = _pairs_refs(case, 1)
        _assert_pairs(_run_pairs(case, 1), want, ref32, "up=1e-3 E=%d L=%d n=%d" % (E, L, n))
    case = din64.pairs_case(8, 1, 4, True, 6, batch=1025, up=1e-3)
    want, ref32 = _pairs_refs(case, 1)
    _assert_pairs(_run_pairs(case, 1), want, ref32, "up=1e-3 M=1025")
    report("din pairs up=1e-3")


# ---- pool ---------------------------------------------------------------------------------------------------------------------
def _run_pool(case, softmax, want=("dscore", "dh")):
    L_ = _lib()
    lib = L_.lib
    score, h, r = (case[k].cuda() for k in ("score", "h", "r"))
    mask = None if case["mask"] is None else case["mask"].cuda()
    Bn, L, E = h.shape
    weight, out = Guarded(Bn, L), Guarded(Bn, E)
    rc = lib.rbx_din_pool_fwd(_p(score), _p(mask), _p(h), L * E, Bn, L, E, int(softmax), _p(weight.view), _p(out.view), None)
    assert rc == L_.RBX_OK, L_.last_error()
    torch.cuda.synchronize()
    ds = Guarded(Bn, L) if "dscore" in want else None
    dh = Guarded(Bn * L, E) if "dh" in want else None
    view = view_of
    rc = lib.rbx_din_pool_bwd(_p(r), _p(weight.view), _p(mask), _p(h), L * E, Bn, L, E, int(softmax), _p(view(ds)), _p(view(dh)),
                              None)
    assert rc == L_.RBX_OK, L_.last_error()
    torch.cuda.synchronize()
    for name, g in (("weight", weight), ("out", out), ("dscore", ds), ("dh", dh)):
        assert g is None or g.untouched(), "%s: a guard band was written" % name
    return {"weight": weight.view, "out": out.view, "dscore": view(ds), "dh": dh and dh.view.view(Bn, L, E)}


def _assert_pool(got, want, ref32, tag):
    for n in din64.POOL_NAMES:
        if got[n] is not None:
            assert_bar("%s %s" % (n, tag), got[n], want[n], ref32[n])


POOL_FORMS = [(B, 1, 4), (B, 8, 128), (B, 255, 12), (B, 256, 16), (B, 257, 16), (3, 4096, 4)]


@pytest.mark.parametrize("masking", ["none", "random", "one_sample_all_masked", "fractions"])
@pytest.mark.parametrize("batch,L,E", POOL_FORMS)
def test_pool_every_length_form(batch, L, E, masking):
    for softmax in (False, True):
        case = din64.pool_case(batch, L, E, masking, 100 * L + E)
        want, ref32 = din64.pool_reference(case, softmax), din64.pool_reference(case, softmax, torch.float32)
        got = _run_pool(case, softmax)
        tag = "L=%d E=%d %s softmax=%d" % (L, E, masking, softmax)
        _assert_pool(got, want, ref32, tag)
        if case["mask"] is not None:
            assert bool((got["dscore"].cpu()[case["mask"] == 0] == 0).all())        # no gradient reaches a masked score
        if masking == "one_sample_all_masked" and softmax:
            dead = min(3, batch - 1)
            assert torch.equal(got["weight"][dead].cpu(), torch.full((L,), 1.0) / L)
    report("din pool L=%d E=%d %s" % (L, E, masking))


@pytest.mark.parametrize("batch,L,E", [(B, 8, 128), (B, 257, 16), (3, 4096, 4)])
def test_pool_with_one_gradient_not_wanted(batch, L, E):
    for softmax in (False, True):
        case = din64.pool_case(batch, L, E, "random", 3 + L)
        want, ref32 = din64.pool_reference(case, softmax), din64.pool_reference(case, softmax, torch.float32)
        full = _run_pool(case, softmax)
        for names in (("dscore",), ("dh",)):
            got = _run_pool(case, softmax, names)
            _assert_pool(got, want, ref32, "L=%d E=%d softmax=%d only %s" % (L, E, softmax, names[0]))
            assert torch.equal(got[names[0]], full[names[0]])
    report("din pool NULLs L=%d E=%d" % (L, E))


def test_pool_small_upstream_gradient_and_a_peaked_softmax():
    """din64.small_pool_case (the inputs of the host test's mutants), and a softmax with one score 20 above the rest: the
    other positions' dscore is about 1e-8 at a unit gradient."""
    case = din64.small_pool_case()
    want, ref32 = din64.pool_reference(case, True), din64.pool_reference(case, True, torch.float32)
    _assert_pool(_run_pool(case, True), want, ref32, "up=1e-3 L=257 E=16")
    for (L, E) in ((8, 128), (257, 16)):
        case = din64.pool_case(B, L, E, "random", 9, peak=20.0)
        want, ref32 = din64.pool_reference(case, True), din64.pool_reference(case, True, torch.float32)
        _assert_pool(_run_pool(case, True), want, ref32, "peaked L=%d E=%d" % (L, E))
    report("din pool small / peaked")


def test_pool_refuses_a_sequence_past_the_lds_row_and_writes_nothing():
    L_ = _lib()
    lib = L_.lib
    L, E = 4097, 4
    case = din64.pool_case(1, L, E, "none", 1)
    score, h, r = (case[k].cuda() for k in ("score", "h", "r"))
    weight, out, ds, dh = Guarded(1, L), Guarded(1, E), Guarded(1, L), Guarded(L, E)
    for softmax in (0, 1):
        assert lib.rbx_din_pool_fwd(_p(score), None, _p(h), L * E, 1, L, E, softmax, _p(weight.view), _p(out.view),
                                    None) == L_.RBX_ERR_UNSUPPORTED
        assert "4096" in L_.last_error()
        assert lib.rbx_din_pool_bwd(_p(r), _p(score), None, _p(h), L * E, 1, L, E, softmax, _p(ds.view), _p(dh.view),
                                    None) == L_.RBX_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert weight.all_nan() and out.all_nan() and ds.all_nan() and dh.all_nan()
