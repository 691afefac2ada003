"""The scale-aware bar of the float64 comparisons (helper of the GRU / additive attention / capsule form tests, not a test).

For one result tensor: ``got`` is the result under test, ``want`` the float64 restatement, ``ref32`` the same restatement run
in float32 on the CPU with plain torch ops.  With e32 = max|ref32 - want| and scale = max|want| the bar is

    max|got - want| <= max(factor * e32, 2e-6 * scale)        factor = 4 unless a test documents another one

-- the rule of the split-operand GEMMs (``_assert_split_accuracy`` in tests/test_gpu_dense_routes.py), per tensor: what fp32
itself loses on these very inputs, times a margin for another summation order, with a floor of a few fp32 roundings of the
largest element for results that fp32 happens to hit exactly.  Nothing ``got`` holds enters the bar.  A gradient of size 1e-3
is held to about 2e-9, where an absolute 1e-4 checks it to 10 %."""
import torch

FACTOR = 4.0
FLOOR = 2e-6
WORST = {}                        # name -> the largest err / bar seen in this process (printed by the form tests)


def _f64(t):
    return t.detach().double().cpu()


def bar_of(want, ref32, factor=FACTOR):
    """(bar, e32, scale) of one tensor."""
    want = _f64(want)
    e32 = float((_f64(ref32) - want).abs().max()) if want.numel() else 0.0
    scale = float(want.abs().max()) if want.numel() else 0.0
    return max(factor * e32, FLOOR * scale), e32, scale


def measure(name, got, want, ref32, factor=FACTOR):
    """Prints ``name: err, e32, scale, err / bar`` and returns (err, bar)."""
    assert tuple(got.shape) == tuple(want.shape) == tuple(ref32.shape), \
        "%s: shapes %s / %s / %s" % (name, tuple(got.shape), tuple(want.shape), tuple(ref32.shape))
    bar, e32, scale = bar_of(want, ref32, factor)
    diff = (_f64(got) - _f64(want)).abs()
    err = float(diff.max()) if diff.numel() else 0.0
    if err != err or not torch.isfinite(_f64(got)).all():
        err = float("inf")
    ratio = err / bar if bar > 0 else (0.0 if err == 0 else float("inf"))
    print("%s: err %.3e e32 %.3e scale %.3e err/bar %.3f" % (name, err, e32, scale, ratio))
    key = name.split(" ")[0]
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    return err, bar


def assert_bar(name, got, want, ref32, factor=FACTOR):
    err, bar = measure(name, got, want, ref32, factor)
    assert err <= bar, "%s: max abs err %.3e > bar %.3e" % (name, err, bar)


def within_bar(got, want, ref32, factor=FACTOR):
    bar, _, _ = bar_of(want, ref32, factor)
    diff = (_f64(got) - _f64(want)).abs()
    return bool(torch.isfinite(_f64(got)).all()) and (float(diff.max()) if diff.numel() else 0.0) <= bar


def within_absolute(got, want, tol=1e-4):
    """The old rule: one absolute bar whatever the tensor's magnitude."""
    diff = (_f64(got) - _f64(want)).abs()
    return (float(diff.max()) if diff.numel() else 0.0) <= tol


def report(tag):
    """One line with the worst err / bar per tensor name since the last report."""
    print("%s worst err/bar: %s" % (tag, ", ".join("%s %.3f" % (k, v) for k, v in sorted(WORST.items()))))
    WORST.clear()
