"""Caser's convolutional layers: forward and forward + backward through (a) the fused op (ops.caser_conv: csrc/rbx_caser.hip) and
(b) the composition (ops.caser_conv_torch: a Conv2d, a ReLU and a max_pool1d per height, two cats), same GPU, same process, same
data; peak memory of both forms.

    python profiles/caser.py --resources     # no GPU: VGPR / SGPR / LDS / scratch figures -> profiles/caser/resources.txt
    python profiles/caser.py --mode fused    # the fused op on its own, all twelve rows
    python profiles/caser.py --mode pair [--rows 0:0,2:1] [--budget SECONDS]   # both forms alternating
    python profiles/caser.py --table-only --out profiles/caser/table.md        # the table of the records so far

Shapes: (L, D, n_h, n_v) = (10, 64, 8, 4), (20, 64, 16, 4), (50, 64, 8, 4), (50, 64, 16, 8) at B = 512, 4096 and 32 768.  Every
row is appended to --log (JSON lines) as soon as it is measured, so rows can be split over several runs; the table takes the
alternating record of a row where there is one and the fused op alone otherwise.  HIP events around ``iters`` steps; both forms
are warmed outside the timed region (the composition's first call at a shape, which includes the convolution library's choice of
a solver for each of its 3 L problems, is timed with the wall clock and listed); (a) and (b) then alternate repetition by
repetition, 5 times; the table gives each form's median and its spread (min .. max over the repetitions).  A speed-up counts as
one only where the two spreads do not overlap.  A composition that runs out of memory is recorded as such."""
import argparse
import contextlib
import json
import os
import re
import subprocess
import sys
import threading
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HERE = os.path.join(ROOT, "profiles", "caser")
SHAPES = ((10, 64, 8, 4), (20, 64, 16, 4), (50, 64, 8, 4), (50, 64, 16, 8))
BATCHES = (512, 4096, 32768)


def resources():
    """Compile csrc/rbx_caser.hip alone with -Rpass-analysis=kernel-resource-usage and tabulate what the compiler reports.  The
    forward takes its LDS dynamically: 4 (T (L D + 4) + max(16 (pad4(L) + 4), 192)) bytes with T = 16 samples, 8 where that
    exceeds 160 KiB (42 240 bytes at 10 x 64, 83 712 at 20 x 64, 106 112 at 50 x 64 with T = 8); the dx kernel 8 L n_h bytes."""
    from recbox_amd import build
    src = os.path.join(build.CSRC, "rbx_caser.hip")
    cmd = [build._hipcc()] + build.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull]
    text = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, check=True).stdout
    rows, cur = [], None
    for line in text.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|AGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|"
                      r"VGPRs Spill|SGPRs Spill|LDS Size \[bytes/block\]):\s+(\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            k = re.search(r"\d+(caser_\w+?_kernel)", m.group(2))
            cur = {"name": k.group(1) if k else m.group(2)}
            rows.append(cur)
        elif cur is not None:
            cur[m.group(1)] = m.group(2)
    lines = ["| kernel | VGPRs | AGPRs | SGPRs | SGPR spills | scratch B/lane | VGPR spills | static LDS B/block | waves/SIMD |",
             "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append("| %s | %s | %s | %s | %s | %s | %s | %s | %s |"
                     % (r["name"], r.get("VGPRs"), r.get("AGPRs"), r.get("TotalSGPRs"), r.get("SGPRs Spill"),
                        r.get("ScratchSize [bytes/lane]"), r.get("VGPRs Spill"), r.get("LDS Size [bytes/block]"),
                        r.get("Occupancy [waves/SIMD]")))
    return "\n".join(lines) + "\n"


def _once(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def _peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2.0 ** 20


def _stats(times, peak):
    t = sorted(times)
    return [t[len(t) // 2], t[0], t[-1], peak]


@contextlib.contextmanager
def _heartbeat(t0, every=60.0):
    """Prints the seconds since t0 once a minute while the body runs: a first call of the composition can take many minutes."""
    done = threading.Event()

    def beat():
        while not done.wait(every):
            print("  ... first call running for %.0f s" % (time.time() - t0), flush=True)
    th = threading.Thread(target=beat, daemon=True)
    th.start()
    try:
        yield
    finally:
        done.set()
        th.join()


def _alone(fn, iters, reps):
    """[median, min, max, peak MiB] of fn measured on its own; the peak run is also the warm-up."""
    peak = _peak(fn)
    return _stats([_once(fn, iters) for _ in range(reps)], peak)


def _pair(fa, fb, iters, reps):
    """([median, min, max, peak MiB] of fa, the same of fb, the seconds fb's first call took).  Both are warmed outside the timed
    region (the composition's first call at a shape includes the convolution library's choice of a solver per problem); then the
    two alternate repetition by repetition.  None for a form that runs out of memory."""
    peaks, warm = [], 0.0
    for fn in (fa, fb):
        try:
            t0 = time.time()
            with _heartbeat(t0):
                fn()
                torch.cuda.synchronize()
            warm = time.time() - t0
            peaks.append(_peak(fn))
        except torch.cuda.OutOfMemoryError:
            torch.cuda.empty_cache()
            peaks.append(None)
    times = ([], [])
    for _ in range(reps):
        for i, fn in enumerate((fa, fb)):
            if peaks[i] is not None:
                times[i].append(_once(fn, iters))
    return [None if peaks[i] is None else _stats(times[i], peaks[i]) for i in range(2)] + [warm]


def _inputs(B, L, D, n_h, n_v):
    g = torch.Generator().manual_seed(B + L + D + n_h)
    x = torch.randn(B, L, D, generator=g).cuda().requires_grad_()
    w_v = (torch.randn(n_v, 1, L, 1, generator=g) / L ** 0.5).cuda().requires_grad_()
    b_v = torch.randn(n_v, generator=g).cuda().requires_grad_()
    w_h = [(torch.randn(n_h, 1, h, D, generator=g) / (h * D) ** 0.5).cuda().requires_grad_() for h in range(1, L + 1)]
    b_h = [(torch.randn(n_h, generator=g) * 0.5).cuda().requires_grad_() for _ in range(L)]
    up = torch.randn(B, n_v * D + n_h * L, generator=g).cuda()
    return (x, w_v, b_v, w_h, b_h), up


def measure(todo, mode, log, budget):
    """One record per (shape, B) of ``todo``, appended to ``log`` as a JSON line as soon as it exists.  mode "fused": the fused op
    on its own; mode "pair": both forms alternating, rows in ascending order of work, and no new row is started once ``budget``
    seconds have passed (a row left out is listed as not measured against the composition)."""
    from recbox_amd import ops
    ops.CASER_FUSED_MAX_LEN, ops.CASER_FUSED_MAX_BATCH = ops.CASER_MAX_LEN, 1 << 40   # measure the kernels over their whole range
    ops.CASER_FUSED_LONG_MAX_BATCH = 1 << 40
    ops.config.caser_fused = True
    start = time.time()

    def work(row):
        (L, D, n_h, n_v), B = row
        return B * L * L * D * n_h
    for row in sorted(todo, key=work):
        if mode == "pair" and time.time() - start > budget:
            print("budget spent before", row, flush=True)
            continue
        shape, B = row
        args, up = _inputs(B, *shape)
        leaves = [args[0], args[1], args[2]] + args[3] + args[4]

        def fwd(fn):
            with torch.no_grad():
                fn(*args)

        def step(fn):
            torch.autograd.grad((fn(*args) * up).sum(), leaves)

        iters = 10 if work(row) < 2e9 else (3 if work(row) < 2e10 else 1)
        print("row", row, mode, flush=True)
        rec = {"shape": list(shape), "B": B, "mode": mode, "iters": iters}
        if mode == "fused":
            rec["fwd"] = [_alone(lambda: fwd(ops.caser_conv), iters, 5), None]
            rec["step"] = [_alone(lambda: step(ops.caser_conv), iters, 5), None]
        else:
            f = _pair(lambda: fwd(ops.caser_conv), lambda: fwd(ops.caser_conv_torch), iters, 5)
            print("  composition forward warmed in %.1f s" % f[2], flush=True)
            s = _pair(lambda: step(ops.caser_conv), lambda: step(ops.caser_conv_torch), iters, 5)
            print("  composition forward + backward warmed in %.1f s" % s[2], flush=True)
            rec.update(fwd=f[:2], step=s[:2], warm_fwd_s=f[2], warm_step_s=s[2])
        print(json.dumps(rec), flush=True)
        if log:
            with open(log, "a") as fh:
                fh.write(json.dumps(rec) + "\n")
        del args, up, leaves
        torch.cuda.empty_cache()


def table(log):
    """The table of the records in ``log``: per (shape, B) the alternating record where there is one, else the fused op alone."""
    best = {}
    with open(log) as fh:
        for line in fh:
            r = json.loads(line)
            key = (tuple(r["shape"]), r["B"])
            if key not in best or r["mode"] == "pair":
                best[key] = r
    lines = ["| L, D, n_h, n_v | B | fused fwd / peak | composition fwd / peak | fwd speed-up | fused fwd+bwd / peak | "
             "composition fwd+bwd / peak | fwd+bwd speed-up | composition's first fwd+bwd call |", "|---|---|---|---|---|---|---|---|---|"]
    for shape in SHAPES:
        for B in BATCHES:
            r = best.get((shape, B))
            if r is None:
                continue
            f, s = r["fwd"], r["step"]
            alone = r["mode"] == "fused"
            lines.append("| %s | %d | %s | %s | %s | %s | %s | %s | %s |"
                         % (", ".join(str(v) for v in shape), B, _cell(f[0]), _cell(f[1], alone), _speed(f[0], f[1]), _cell(s[0]),
                            _cell(s[1], alone), _speed(s[0], s[1]), "n/a" if alone else "%.1f s" % r["warm_step_s"]))
    return "\n".join(lines) + "\n"


def _cell(r, alone=False):
    if r is None:
        return "not measured (fused alone)" if alone else "out of memory"
    return "%.3f (%.3f .. %.3f) ms / %.0f MiB" % tuple(r)


def _speed(a, b):
    if a is None or b is None:
        return "n/a"
    clear = a[2] < b[1] or b[2] < a[1]
    return "%.2fx%s" % (b[0] / a[0], "" if clear else " (within the spread)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--mode", choices=("fused", "pair"), default="pair")
    ap.add_argument("--rows", default=None, help="shape:batch indices, e.g. 0:0,2:1 (default: all twelve)")
    ap.add_argument("--budget", type=float, default=1e9, help="seconds after which --mode pair starts no further row")
    ap.add_argument("--log", default=os.path.join(HERE, "rows.jsonl"), help="JSON lines, appended to")
    ap.add_argument("--out", default=None, help="write the table of --log here (with no other work when --table-only)")
    ap.add_argument("--table-only", action="store_true")
    a = ap.parse_args()
    if a.resources:
        text = resources()
        os.makedirs(HERE, exist_ok=True)
        with open(os.path.join(HERE, "resources.txt"), "w") as fh:
            fh.write(text)
        print(text)
        return
    if not a.table_only:
        todo = [(s, b) for s in SHAPES for b in BATCHES]
        if a.rows:
            todo = [(SHAPES[int(i)], BATCHES[int(j)]) for i, j in (p.split(":") for p in a.rows.split(","))]
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        measure(todo, a.mode, a.log, a.budget)
    text = table(a.log)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
