"""DCN-V2's cross expert mixture: forward + backward of the layer stack through (a) the fused op (ops.cross_mix:
csrc/rbx_crossmix.hip) and (b) the composition (ops.cross_mix_torch), same GPU, same process, same data; each C-ABI call alone
(ops.kernel_timer) against its byte and FLOP counts; peak memory of both forms; one DCNv2 (parallel, mixture) step.

    python profiles/crossmix.py --resources     # no GPU: VGPR / SGPR / LDS / scratch figures -> profiles/crossmix/resources.txt
    python profiles/crossmix.py [--out profiles/crossmix/table.md] [--quick]

Shapes: B = 4096 and 65 536, n = 26 x 16 and 39 x 16, E = 4, r = 32 and 8, L = 2 and 3 (--quick: B = 4096, n = 416 only).  HIP
events around ``iters`` steps after a warm-up, median of ``reps`` repetitions, (a) and (b) alternating.  Per layer and sample
(fp32): the forward's irreducible traffic is x_l and x0 read and out written, 12 n bytes, and its MFMA work 2 n (2 E r + E)
FLOP; the backward row launch reads x_l, x0, dout and writes dx_l, dx0 (20 n bytes, dx0 read again when it accumulates) plus
the 16 E r + 4 E bytes of weight-gradient operands, and runs 2 n 4 E r FLOP.  Byte share = those bytes over the call's time
over 8 TB/s; MFMA share = those FLOP over the call's time over 157 TFLOP/s (the fp32 matrix peak)."""
import argparse
import os
import re
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HERE = os.path.join(ROOT, "profiles", "crossmix")
HBM_PEAK, MFMA_PEAK = 8.0e12, 157.0e12


def resources():
    """Compile csrc/rbx_crossmix.hip alone with -Rpass-analysis=kernel-resource-usage and tabulate what the compiler reports."""
    from recbox_amd import build
    src = os.path.join(build.CSRC, "rbx_crossmix.hip")
    cmd = [build._hipcc()] + build.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull]
    text = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, check=True).stdout
    rows, cur = [], None
    for line in text.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|AGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|"
                      r"VGPRs Spill|LDS Size \[bytes/block\]):\s+(\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            k = re.search(r"\d+(cm_\w+?_kernel)", m.group(2))
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


def _case(B, n, E, r, L, iters, reps):
    from recbox_amd import ops
    g = torch.Generator().manual_seed(1)
    leaf = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).cuda().requires_grad_()      # noqa: E731
    x0, G = leaf(B, n), leaf(E, n, scale=n ** -0.5)
    U = [leaf(E, n, r, scale=r ** -0.5) for _ in range(L)]
    V = [leaf(E, n, r, scale=n ** -0.5) for _ in range(L)]
    C = [leaf(E, r, r, scale=r ** -0.5) for _ in range(L)]
    b = [leaf(n, 1, scale=0.1) for _ in range(L)]
    up = torch.randn(B, n, device="cuda")
    leaves = [x0, G] + U + V + C + b

    def step(op):
        def run():
            torch.autograd.grad(op(x0, U, V, C, G, b), leaves, up)
        return run

    # the kernels are timed at every shape, also where ops.cross_mix would hand the call to the composition
    ops.CROSSMIX_MAX_BATCH = ops.CROSSMIX_MAX_WORK = 1 << 62
    fused, comp = step(ops.cross_mix), step(ops.cross_mix_torch)
    ms = _median_ms([fused, comp], iters, reps)
    timer = _Timer()
    ops.kernel_timer = timer
    try:
        for _ in range(3):
            fused()
        calls = timer.totals()
    finally:
        ops.kernel_timer = None
    er = E * r
    fwd_us, bwd_us = calls["crossmix_fwd"], calls["crossmix_bwd"]
    return {"fused": ms[0], "comp": ms[1], "fwd_us": fwd_us, "bwd_us": bwd_us,
            "fwd_bytes": 12.0 * B * n / (fwd_us * 1e-6) / HBM_PEAK,
            "fwd_flop": 2.0 * B * n * (2 * er + E) / (fwd_us * 1e-6) / MFMA_PEAK,
            "bwd_bytes": B * (20.0 * n + 16.0 * er + 4.0 * E) / (bwd_us * 1e-6) / HBM_PEAK,
            "bwd_flop": 2.0 * B * n * 4 * er / (bwd_us * 1e-6) / MFMA_PEAK,
            "peak_fused": _peak(fused) / (4.0 * B * n), "peak_comp": _peak(comp) / (4.0 * B * n)}


def _model_step(iters, reps):
    """One DCNv2 step (parallel, mixture: 26 x 16, B = 4096, 3 cross layers, low_rank 32, 4 experts, MLP [256, 128])."""
    from recbox_amd import ops
    from recbox_amd.rechub.basic.features import SparseFeature
    from recbox_amd.rechub.models.ranking import DCNv2
    feats = [SparseFeature("c%d" % i, vocab_size=1000, embed_dim=16) for i in range(26)]
    model = DCNv2(feats, 3, {"dims": [256, 128], "activation": "relu", "dropout": 0.0}).cuda().train()
    g = torch.Generator().manual_seed(2)
    x = {"c%d" % i: torch.randint(0, 1000, (4096,), generator=g).cuda() for i in range(26)}
    old = ops.config.check_ids
    ops.config.check_ids = False

    def step(flag):
        def run():
            ops.config.crossmix_fused = flag
            for p in model.parameters():
                p.grad = None
            model(x).sum().backward()
        return run
    try:
        return _median_ms([step(True), step(False)], iters, reps)
    finally:
        ops.config.crossmix_fused, ops.config.check_ids = True, old


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(HERE, "table.md"))
    a = ap.parse_args()
    if a.resources:
        os.makedirs(HERE, exist_ok=True)
        with open(os.path.join(HERE, "resources.txt"), "w") as fh:
            fh.write(resources())
        print(open(os.path.join(HERE, "resources.txt")).read())
        return
    lines = ["| B | n | E | r | L | fused ms | composition ms | composition / fused | fwd us / layer (byte share, MFMA share) | "
             "bwd us / layer (byte share, MFMA share) | peak fused / [B, n] | peak composition / [B, n] |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for B in ((4096,) if a.quick else (4096, 65536)):
        for n in ((416,) if a.quick else (416, 624)):
            for r in (32, 8):
                for L in (2, 3):
                    q = _case(B, n, 4, r, L, a.iters, a.reps)
                    lines.append("| %d | %d | 4 | %d | %d | %.3f | %.3f | %.2fx | %.1f (%.3f, %.3f) | %.1f (%.3f, %.3f) | %.2f | %.2f |"
                                 % (B, n, r, L, q["fused"], q["comp"], q["comp"] / q["fused"], q["fwd_us"], q["fwd_bytes"],
                                    q["fwd_flop"], q["bwd_us"], q["bwd_bytes"], q["bwd_flop"], q["peak_fused"], q["peak_comp"]))
                    print(lines[-1], flush=True)
                    torch.cuda.empty_cache()
    fused, comp = _model_step(a.iters, a.reps)
    lines += ["", "DCNv2 step (parallel, mixture; B = 4096, 26 x 16, 3 cross layers, low_rank 32, 4 experts, MLP [256, 128]): "
              "fused %.3f ms, composition %.3f ms (%.2fx)." % (fused, comp, comp / fused)]
    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
