"""Expert-gate mixing of the multi-task models: forward + backward of (a) the fused op (ops.expert_mix: csrc/rbx_mix.hip) and
(b) the composition it replaces (ops.expert_mix_torch: torch.cat / torch.mul / torch.sum per gate), same GPU, same process,
same data; and each kernel alone against its byte count.

    python profiles/expert_mix.py --resources     # no GPU: the kernels' VGPR / SGPR / LDS / scratch figures -> profiles/expert_mix/resources.txt
    python profiles/expert_mix.py [--out profiles/expert_mix/INDEX.md]

Shapes: MMOE's form (every gate over all experts) at (E, H, T) = (8, 128, 3) and (4, 64, 2), PLE's selection with 2 specific + 1
shared experts and 3 tasks (+ the shared gate: E = 7, T = 4), AITM's (2, 32, 1) over two interleaved rows of one [B, 2, H]
tensor, each at B = 65 536 and B = 8 192.  HIP events around ``iters`` steps after a warm-up, median of ``reps`` repetitions, (a)
and (b) alternating.  Bytes a kernel must move (fp32): forward reads E H + sum n_t and writes T H + sum n_t per sample; backward
reads E H + T H + sum n_t and writes E H + sum n_t.  Share of peak = those bytes over the kernel's time over 8 TB/s."""
import argparse
import os
import re
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HERE = os.path.join(ROOT, "profiles", "expert_mix")
HBM_PEAK = 8.0e12


def resources():
    """Compile csrc/rbx_mix.hip alone with -Rpass-analysis=kernel-resource-usage and tabulate what the compiler reports."""
    from recbox_amd import build
    src = os.path.join(build.CSRC, "rbx_mix.hip")
    cmd = [build._hipcc()] + build.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull]
    text = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, check=True).stdout
    rows, cur = [], None
    for line in text.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|AGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|"
                      r"VGPRs Spill|LDS Size \[bytes/block\]):\s+(\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            k = re.search(r"mix_(fwd|bwd)_kernelILi(\d+)E(?:Li(\d+)E)?", m.group(2))
            name = m.group(2)
            if k:
                name = "mix_%s_kernel<%s>" % (k.group(1), ", ".join(g for g in k.groups()[1:] if g))
            cur = {"name": name}
            rows.append(cur)
        elif cur is not None:
            cur[m.group(1)] = m.group(2)
    lines = ["| kernel (fwd: <columns per lane>; bwd: <lane group, columns per lane>) | VGPRs | AGPRs | SGPRs | scratch B/lane | "
             "VGPR spills | LDS B/block | waves/SIMD |", "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append("| %s | %s | %s | %s | %s | %s | %s | %s |" % (r["name"], r.get("VGPRs"), r.get("AGPRs"), r.get("TotalSGPRs"),
                                                                   r.get("ScratchSize [bytes/lane]"), r.get("VGPRs Spill"),
                                                                   r.get("LDS Size [bytes/block]"),
                                                                   r.get("Occupancy [waves/SIMD]")))
    return "\n".join(lines) + "\n"


def _median_ms(fns, iters, reps):
    """Median ms per call of every fn, the fns alternating inside each repetition."""
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


def _case(form, B, E, H, select, interleaved, iters, reps):
    from recbox_amd import ops
    g = torch.Generator().manual_seed(1)
    T, n_sum = len(select), sum(len(s) for s in select)
    if interleaved:
        base = torch.randn(B, E, H, generator=g).cuda().requires_grad_(True)
        xs, x_leaves = [base[:, e] for e in range(E)], [base]
    else:
        xs = [torch.randn(B, H, generator=g).cuda().requires_grad_(True) for _ in range(E)]
        x_leaves = xs
    zs = [torch.randn(B, len(s), generator=g).cuda().requires_grad_(True) for s in select]
    ups = [torch.randn(B, H, generator=g).cuda() for _ in select]
    leaves = x_leaves + zs

    def step(fn):
        def run():
            outs = fn(xs, zs, select, True)
            torch.autograd.grad(outs, leaves, ups)
        return run

    def fwd_only():
        with torch.no_grad():
            ops.expert_mix(xs, zs, select, True)

    fused, comp, fwd = _median_ms([step(ops.expert_mix), step(ops.expert_mix_torch), fwd_only], iters, reps)
    bwd = max(fused - fwd, 1e-9)                        # the fused step is exactly the two launches (+ autograd's bookkeeping)
    fwd_bytes = 4.0 * B * (E * H + T * H + 2 * n_sum)
    bwd_bytes = 4.0 * B * (2 * E * H + T * H + 2 * n_sum)
    return {"fused": fused, "comp": comp, "fwd": fwd, "bwd": bwd,
            "fwd_share": fwd_bytes / (fwd * 1e-3) / HBM_PEAK, "bwd_share": bwd_bytes / (bwd * 1e-3) / HBM_PEAK,
            "fwd_gb": fwd_bytes / 1e9, "bwd_gb": bwd_bytes / 1e9}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(HERE, "INDEX.md"))
    a = ap.parse_args()
    res_path = os.path.join(HERE, "resources.txt")
    if a.resources:
        os.makedirs(HERE, exist_ok=True)
        with open(res_path, "w") as fh:
            fh.write(resources())
        print(open(res_path).read())
        return
    ple = [[0, 1, 6], [2, 3, 6], [4, 5, 6], list(range(7))]
    forms = [("MMOE", 8, 128, [list(range(8))] * 3, False), ("MMOE", 4, 64, [list(range(4))] * 2, False),
             ("PLE 2 + 1, 3 tasks, H = 128", 7, 128, ple, False), ("PLE 2 + 1, 3 tasks, H = 64", 7, 64, ple, False),
             ("AITM (interleaved rows)", 2, 32, [[0, 1]], True)]
    lines = ["# Expert-gate mixing: fused op (csrc/rbx_mix.hip) against the cat / mul / sum composition, forward + backward", "",
             "Written by `python profiles/expert_mix.py` on %s; median of %d x %d steps, HIP events, (a) and (b) alternating.  "
             "The kernel columns: the forward alone (timed under no_grad) and the fused step minus it; their share of the HBM "
             "peak (%.0f TB/s) is the bytes the kernel must move over its time." % (torch.cuda.get_device_name(0), a.reps, a.iters,
                                                                                  HBM_PEAK / 1e12), "",
             "| form | B | E | H | T | (a) fused ms | (b) composition ms | (b) / (a) | fwd kernel ms | fwd GB | fwd share of peak | "
             "bwd kernel ms | bwd GB | bwd share of peak |", "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for B in (65536, 8192):
        for form, E, H, select, inter in forms:
            r = _case(form, B, E, H, select, inter, a.iters, a.reps)
            lines.append("| %s | %d | %d | %d | %d | %.3f | %.3f | %.2f x | %.3f | %.3f | %.0f %% | %.3f | %.3f | %.0f %% |"
                         % (form, B, E, H, len(select), r["fused"], r["comp"], r["comp"] / r["fused"], r["fwd"], r["fwd_gb"],
                            100 * r["fwd_share"], r["bwd"], r["bwd_gb"], 100 * r["bwd_share"]))
            print(lines[-1], flush=True)
            torch.cuda.empty_cache()
    lines += ["", "## Compiler resource figures (hipcc -Rpass-analysis=kernel-resource-usage, gfx950)", ""]
    lines.append(open(res_path).read() if os.path.exists(res_path) else resources())
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
