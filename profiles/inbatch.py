"""In-batch band scores: forward + backward through (a) the fused op (ops.inbatch_band_scores: csrc/rbx_inbatch.hip), (b) the
gather composition (ops.inbatch_band_scores_torch) and, where it fits in memory (B = 4096), (c) the reference's literal form
(torch.cosine_similarity broadcast to [B, B, D], - log w, [index0, index1], / temperature); same GPU, same process, same data;
each C-ABI call alone (ops.kernel_timer) against its byte count; peak memory of every form.

    python profiles/inbatch.py --resources     # no GPU: VGPR / SGPR / LDS / scratch figures -> profiles/inbatch/resources.txt
    python profiles/inbatch.py [--out profiles/inbatch/table.md] [--quick]

Shapes: B = 4096 and 65 536, D = 32 / 64 / 128, n_neg = 3 and 31, with sample weights (--quick: B = 4096, D = 64 only).  HIP
events around ``iters`` steps after a warm-up, median of ``reps`` repetitions, the forms alternating.  By hand (fp32): the forward
must read u and v and write the scores, 2 B D 4 + B (n_neg + 1) 4 bytes; the backward reads u, v and g and writes du and dv,
(2 + 2) B D 4 + B (n_neg + 1) 4 bytes.  Byte share = those bytes over the call's time over 8 TB/s."""
import argparse
import os
import re
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HERE = os.path.join(ROOT, "profiles", "inbatch")
HBM_PEAK = 8.0e12


def resources():
    """Compile csrc/rbx_inbatch.hip alone with -Rpass-analysis=kernel-resource-usage and tabulate what the compiler reports."""
    from recbox_amd import build
    src = os.path.join(build.CSRC, "rbx_inbatch.hip")
    cmd = [build._hipcc()] + build.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull]
    text = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, check=True).stdout
    rows, cur = [], None
    for line in text.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|AGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|"
                      r"VGPRs Spill|LDS Size \[bytes/block\]):\s+(\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            k = re.search(r"\d+(ib_\w+?_kernel)", m.group(2))
            cur = {"name": k.group(1) if k else m.group(2)}
            rows.append(cur)
        elif cur is not None:
            cur[m.group(1)] = m.group(2)
    lines = ["| kernel | VGPRs | AGPRs | SGPRs | scratch B/lane | VGPR spills | static LDS B/block | waves/SIMD |",
             "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append("| %s | %s | %s | %s | %s | %s | %s | %s |" % (r["name"], r.get("VGPRs"), r.get("AGPRs"), r.get("TotalSGPRs"),
                                                                   r.get("ScratchSize [bytes/lane]"), r.get("VGPRs Spill"),
                                                                   r.get("LDS Size [bytes/block]"), r.get("Occupancy [waves/SIMD]")))
    return "\n".join(lines) + "\n"


def _median_ms(fns, iters, reps):
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / iters)
    return [sorted(t)[len(t) // 2] for t in times]


class _Timer(object):
    """ops.kernel_timer: HIP events around every C-ABI call, the median per call name."""

    def __init__(self):
        self.pending = []

    def bracket(self, meta, fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = fn()
        e1.record()
        self.pending.append((meta[0], e0, e1))
        return rc

    def totals(self):
        torch.cuda.synchronize()
        out = {}
        for name, e0, e1 in self.pending:
            out.setdefault(name, []).append(e0.elapsed_time(e1) * 1e3)
        self.pending = []
        return {k: sorted(v)[len(v) // 2] for k, v in out.items()}


def _peak(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def literal(u, v, n_neg, weight, temperature):
    """rechub's YoutubeSBC.forward, from the tower outputs on."""
    B = u.shape[0]
    index0 = np.repeat(np.arange(B), n_neg + 1)
    index1 = np.concatenate([np.arange(i, i + n_neg + 1) for i in range(B)])
    index1[np.where(index1 >= B)] -= B
    pred = torch.cosine_similarity(u.unsqueeze(1), v, dim=2)
    scores = (pred - torch.log(weight))[index0, index1] / temperature
    return scores.view(-1, n_neg + 1)


def _case(B, D, n, iters, reps, with_literal):
    from recbox_amd import ops
    g = torch.Generator().manual_seed(1)
    u, v = (torch.randn(B, D, generator=g).cuda().requires_grad_() for _ in range(2))
    w = (0.05 + 0.95 * torch.rand(B, generator=g)).cuda()
    up = torch.randn(B, n + 1, generator=g).cuda()

    def step(op):
        def run():
            torch.autograd.grad(op(u, v, n, w, 0.5), [u, v], up)
        return run

    fused, comp = step(ops.inbatch_band_scores), step(ops.inbatch_band_scores_torch)
    forms = [fused, comp] + ([step(literal)] if with_literal else [])
    ms = _median_ms(forms, iters, reps)
    timer = _Timer()
    ops.kernel_timer = timer
    try:
        for _ in range(5):
            fused()
        calls = timer.totals()
    finally:
        ops.kernel_timer = None
    fwd_us, bwd_us = calls["inbatch_band_fwd"], calls["inbatch_band_bwd"]
    band = 4.0 * B * (n + 1)
    return {"ms": ms, "fwd_us": fwd_us, "bwd_us": bwd_us,
            "fwd_share": (8.0 * B * D + band) / (fwd_us * 1e-6) / HBM_PEAK,
            "bwd_share": (16.0 * B * D + band) / (bwd_us * 1e-6) / HBM_PEAK,
            "peak": [_peak(f) / 2.0 ** 20 for f in forms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(HERE, "table.md"))
    a = ap.parse_args()
    if a.resources:
        os.makedirs(HERE, exist_ok=True)
        with open(os.path.join(HERE, "resources.txt"), "w") as fh:
            fh.write(resources())
        print(open(os.path.join(HERE, "resources.txt")).read())
        return
    if not torch.cuda.is_available():
        raise SystemExit("profiles/inbatch.py measures on the GPU; none is visible")
    lines = ["| B | D | n_neg | fused ms | composition ms | composition / fused | literal ms | literal / fused | fwd us (byte share) | "
             "bwd us (byte share) | peak MiB fused | peak MiB composition | peak MiB literal |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for B in ((4096,) if a.quick else (4096, 65536)):
        for D in ((64,) if a.quick else (32, 64, 128)):
            for n in (3, 31):
                lit = B == 4096
                q = _case(B, D, n, a.iters, a.reps, lit)
                ms, peak = q["ms"], q["peak"]
                lines.append("| %d | %d | %d | %.3f | %.3f | %.2fx | %s | %s | %.1f (%.3f) | %.1f (%.3f) | %.2f | %.2f | %s |"
                             % (B, D, n, ms[0], ms[1], ms[1] / ms[0], "%.3f" % ms[2] if lit else "does not fit",
                                "%.1fx" % (ms[2] / ms[0]) if lit else "-", q["fwd_us"], q["fwd_share"], q["bwd_us"],
                                q["bwd_share"], peak[0], peak[1], "%.0f" % peak[2] if lit else "-"))
                print(lines[-1], flush=True)
                torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
