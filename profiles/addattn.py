"""Additive attention pooling of NARM / STAMP: forward + backward of (a) the fused op (ops.additive_attn_pool:
csrc/rbx_addattn.hip) and (b) the ATen composition it replaces (ops.additive_attn_pool_torch), with the peak memory of each.

    python profiles/addattn.py --resources       # no GPU: the kernels' VGPR / LDS / scratch figures -> profiles/addattn/resources.txt
    python profiles/addattn.py [--out profiles/addattn/INDEX.md] [--quick]

Shapes: B = 4096 and 65 536, L = 50, D = H = 16 / 64 / 128, and NARM's (B = 512, L = 20, D = H = 100); ctx given, lengths
uniform in 1 .. L, gradients for x, W, ctx and v.  Same GPU, same process, same data; HIP events around `iters` steps after a
warm-up, median of `reps` repetitions; peak memory = torch.cuda.max_memory_allocated over one step, minus what the inputs hold."""
import argparse
import os
import re
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HERE = os.path.join(ROOT, "profiles", "addattn")


def resources():
    """Compile csrc/rbx_addattn.hip alone with -Rpass-analysis=kernel-resource-usage and tabulate what the compiler reports."""
    from recbox_amd import build
    src = os.path.join(build.CSRC, "rbx_addattn.hip")
    cmd = [build._hipcc()] + build.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull]
    text = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, check=True).stdout
    rows, cur = [], None
    for line in text.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|AGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|"
                      r"VGPRs Spill|LDS Size \[bytes/block\]):\s+(\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            k = re.search(r"addattn_(fwd|bwd)_kernelILi(\d+)E", m.group(2))
            cur = {"name": "addattn_%s_kernel<%s>" % (k.group(1), k.group(2)) if k else
                   ("addattn_dv_kernel" if "addattn_dv_kernel" in m.group(2) else m.group(2))}
            rows.append(cur)
        elif cur is not None:
            cur[m.group(1)] = m.group(2)
    lines = ["| kernel (k-steps laid out: D, H <= 4 x) | VGPRs | AGPRs | SGPRs | scratch B/lane | VGPR spills | LDS B/block | waves/SIMD |",
             "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append("| %s | %s | %s | %s | %s | %s | %s | %s |" % (r["name"], r.get("VGPRs"), r.get("AGPRs"), r.get("TotalSGPRs"),
                                                                   r.get("ScratchSize [bytes/lane]"), r.get("VGPRs Spill"),
                                                                   r.get("LDS Size [bytes/block]"),
                                                                   r.get("Occupancy [waves/SIMD]")))
    return "\n".join(lines) + "\n"


def _time(fn, iters, reps):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / iters)
    return sorted(times)[len(times) // 2]


def _case(B, L, D, H, iters, reps):
    from recbox_amd import ops
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, L, D, generator=g).cuda().requires_grad_(True)
    w = (torch.randn(H, D, generator=g) / D ** 0.5).cuda().requires_grad_(True)
    c = torch.randn(B, H, generator=g).cuda().requires_grad_(True)
    v = (torch.randn(H, generator=g) / H ** 0.5).cuda().requires_grad_(True)
    lengths = torch.randint(1, L + 1, (B,), generator=g)
    mask = (torch.arange(L).unsqueeze(0) < lengths.unsqueeze(1)).cuda()
    up = torch.randn(B, D, generator=g).cuda()
    leaves = [x, w, c, v]

    def step(fn):
        def run():
            out, _ = fn(x, w, c, v, mask, 0.0)
            torch.autograd.grad((out * up).sum(), leaves)
        return run

    res = {}
    for tag, fn in (("fused", step(ops.additive_attn_pool)), ("composition", step(ops.additive_attn_pool_torch))):
        try:
            res[tag] = _time(fn, iters, reps)
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            fn()
            torch.cuda.synchronize()
            res[tag + "_mem"] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
        except torch.cuda.OutOfMemoryError:
            res[tag] = res[tag + "_mem"] = None
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--quick", action="store_true", help="leave B = 65 536 out")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(HERE, "INDEX.md"))
    a = ap.parse_args()
    res_path = os.path.join(HERE, "resources.txt")
    if a.resources:
        os.makedirs(HERE, exist_ok=True)
        with open(res_path, "w") as fh:
            fh.write(resources())
        print(open(res_path).read())
        return
    cases = [(B, 50, H, H) for B in ([4096] if a.quick else [4096, 65536]) for H in (16, 64, 128)]
    cases.append((512, 20, 100, 100))
    lines = ["# Additive attention pooling: fused op (csrc/rbx_addattn.hip) against the ATen composition, forward + backward", "",
             "Written by `python profiles/addattn.py` on %s; median of %d x %d steps, HIP events; peak MiB of one step above the"
             % (torch.cuda.get_device_name(0), a.reps, a.iters), "inputs.", "",
             "| B | L | D | H | (a) fused ms | (b) composition ms | (b) / (a) | (a) peak MiB | (b) peak MiB |",
             "|---|---|---|---|---|---|---|---|---|"]

    def num(v, fmt):
        return fmt % v if v is not None else "not measured (out of memory)"
    for B, L, D, H in cases:
        r = _case(B, L, D, H, a.iters, a.reps)
        ratio = "%.2f x" % (r["composition"] / r["fused"]) if (r["fused"] and r["composition"]) else "-"
        lines.append("| %d | %d | %d | %d | %s | %s | %s | %s | %s |"
                     % (B, L, D, H, num(r["fused"], "%.3f"), num(r["composition"], "%.3f"), ratio, num(r["fused_mem"], "%.1f"),
                        num(r["composition_mem"], "%.1f")))
        print(lines[-1], flush=True)
    lines += ["", "Not measured: other L, widths between those, D != H, each kernel alone against its fp32-MFMA / HBM bound, and the",
              "models end to end.", "",
              "## Compiler resource figures (hipcc -Rpass-analysis=kernel-resource-usage, gfx950)", ""]
    lines.append(open(res_path).read() if os.path.exists(res_path) else resources())
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
