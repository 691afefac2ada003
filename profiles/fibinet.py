"""FiBiNet's SENET gate + bilinear pairs: forward + backward of (a) the fused ops (ops.senet_gate, ops.bilinear_pairs(scale=a):
csrc/rbx_bilinear.hip) and (b) the composition (ops.senet_gate_torch, ops.bilinear_pairs_torch), same GPU, same process, same
data; each C-ABI call alone (ops.kernel_timer) against its byte count; peak memory of both forms; the full FiBiNet step.

    python profiles/fibinet.py --resources     # no GPU: VGPR / SGPR / LDS / scratch figures -> profiles/fibinet/resources.txt
    python profiles/fibinet.py [--out profiles/fibinet/table.md] [--quick]

Shapes: B = 4096 and 65 536, F = 26 and 39, D = 8, 16, 32, the three kinds (--quick: B = 4096, F = 26 only).  A shape whose
composition would need more than ``--budget`` GB ([B, 2P, D] x 10 tensors of that size) is skipped for the composition and says
so.  HIP events around ``iters`` steps after a warm-up, median of ``reps`` repetitions, (a) and (b) alternating.  Bytes (fp32)
per sample: forward F 4D read + 2P 4D written; backward 2P 4D + F 4D read, F 4D written, plus the dW partials
(chunks P D D 4 bytes in all, written and read once).  Share = those bytes over the call's time over 8 TB/s."""
import argparse
import os
import re
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HERE = os.path.join(ROOT, "profiles", "fibinet")
HBM_PEAK = 8.0e12
KINDS = ("field_all", "field_each", "field_interaction")


def resources():
    """Compile csrc/rbx_bilinear.hip alone with -Rpass-analysis=kernel-resource-usage and tabulate what the compiler reports."""
    from recbox_amd import build
    src = os.path.join(build.CSRC, "rbx_bilinear.hip")
    cmd = [build._hipcc()] + build.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull]
    text = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, check=True).stdout
    rows, cur = [], None
    for line in text.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|AGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|"
                      r"VGPRs Spill|LDS Size \[bytes/block\]):\s+(\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            k = re.search(r"\d+(gate_\w+?_kernel|bl_\w+?_kernel)(?:ILi(\d+)E)?", m.group(2))
            cur = {"name": ("%s<D = %s>" % (k.group(1), k.group(2)) if k and k.group(2) else (k.group(1) if k else m.group(2)))}
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
    """ops.kernel_timer: HIP events around every C-ABI call, summed per call name."""

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


def _case(B, F, D, kind, iters, reps, budget):
    from recbox_amd import _lib, ops
    g = torch.Generator().manual_seed(1)
    P, R = F * (F - 1) // 2, max(1, F // 3)
    M = (1, F, P)[KINDS.index(kind)]
    x = torch.randn(B, F, D, generator=g).cuda().requires_grad_()
    w1 = (torch.randn(R, F, generator=g) * 0.3).cuda().requires_grad_()
    w2 = (torch.randn(F, R, generator=g) * 0.3).cuda().requires_grad_()
    W = (torch.randn(M, D, D, generator=g) * 0.3).cuda().requires_grad_()
    up = torch.randn(B, 2 * P, D, device="cuda")
    block = 4.0 * B * 2 * P * D

    def step(gate, pairs):
        def run():
            out = pairs(x, W, kind, False, gate(x, w1, w2, "relu"))
            torch.autograd.grad(out, (x, w1, w2, W), up)
        return run

    fused = step(ops.senet_gate, ops.bilinear_pairs)
    comp = step(ops.senet_gate_torch, ops.bilinear_pairs_torch) if 10 * block <= budget * 1e9 else None
    ms = _median_ms([fused] + ([comp] if comp else []), iters, reps)
    timer = _Timer()
    ops.kernel_timer = timer
    try:
        for _ in range(3):
            fused()
        calls = timer.totals()
    finally:
        ops.kernel_timer = None
    part = _lib.lib.rbx_bilinear_pairs_bwd_workspace_size(B, F, D)
    fwd_bytes = 4.0 * B * D * (F + 2 * P)
    bwd_bytes = 4.0 * B * D * (2 * P + 2 * F) + 2.0 * part
    r = {"fused": ms[0], "comp": ms[1] if comp else None, "calls": calls,
         "fwd_share": fwd_bytes / (calls["bilinear_pairs_fwd"] * 1e-6) / HBM_PEAK,
         "bwd_share": bwd_bytes / (calls["bilinear_pairs_bwd"] * 1e-6) / HBM_PEAK,
         "peak_fused": _peak(fused) / block, "peak_comp": _peak(comp) / block if comp else None}
    return r


def _model_step(iters, reps):
    """The full FiBiNet step at Criteo's 26 x 16, B = 4096: lookup, gate, pairs, MLP [256, 128], loss, backward."""
    from recbox_amd import ops
    from recbox_amd.rechub.basic.features import SparseFeature
    from recbox_amd.rechub.models.ranking import FiBiNet
    feats = [SparseFeature("c%d" % i, vocab_size=1000, embed_dim=16) for i in range(26)]
    model = FiBiNet(feats, {"dims": [256, 128], "activation": "relu", "dropout": 0.0}).cuda().train()
    g = torch.Generator().manual_seed(2)
    x = {"c%d" % i: torch.randint(0, 1000, (4096,), generator=g).cuda() for i in range(26)}
    old = ops.config.check_ids
    ops.config.check_ids = False

    def step(flag):
        def run():
            ops.config.bilinear_fused = flag
            for p in model.parameters():
                p.grad = None
            model(x).sum().backward()
        return run
    try:
        return _median_ms([step(True), step(False)], iters, reps)
    finally:
        ops.config.bilinear_fused, ops.config.check_ids = True, old


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--budget", type=float, default=100.0)
    ap.add_argument("--out", default=os.path.join(HERE, "table.md"))
    a = ap.parse_args()
    if a.resources:
        os.makedirs(HERE, exist_ok=True)
        with open(os.path.join(HERE, "resources.txt"), "w") as fh:
            fh.write(resources())
        print(open(os.path.join(HERE, "resources.txt")).read())
        return
    lines = ["| B | F | D | kind | fused ms | composition ms | composition / fused | gate fwd us | pairs fwd us (share) | "
             "pairs bwd us (share) | gate bwd us | peak fused / block | peak composition / block |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for B in ((4096,) if a.quick else (4096, 65536)):
        for F in ((26,) if a.quick else (26, 39)):
            for D in (8, 16, 32):
                for kind in KINDS:
                    r = _case(B, F, D, kind, a.iters, a.reps, a.budget)
                    c = r["calls"]
                    lines.append("| %d | %d | %d | %s | %.3f | %s | %s | %.1f | %.1f (%.2f) | %.1f (%.2f) | %.1f | %.2f | %s |"
                                 % (B, F, D, kind, r["fused"], "%.3f" % r["comp"] if r["comp"] else "skipped (memory)",
                                    "%.2fx" % (r["comp"] / r["fused"]) if r["comp"] else "-", c["senet_gate_fwd"],
                                    c["bilinear_pairs_fwd"], r["fwd_share"], c["bilinear_pairs_bwd"], r["bwd_share"],
                                    c["senet_gate_bwd"], r["peak_fused"], "%.2f" % r["peak_comp"] if r["peak_comp"] else "-"))
                    print(lines[-1], flush=True)
                    torch.cuda.empty_cache()
    fused, comp = _model_step(a.iters, a.reps)
    lines += ["", "Full FiBiNet step (B = 4096, 26 x 16, field_interaction, MLP [256, 128]): fused %.3f ms, composition %.3f ms "
              "(%.2fx)." % (fused, comp, comp / fused)]
    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
