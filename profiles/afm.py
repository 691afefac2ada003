"""AFM's pair-attention pooling: forward + backward through (a) the fused op (ops.afm_pool: csrc/rbx_afm.hip) and (b) the
composition (ops.afm_pool_torch), same GPU, same process, same data; peak memory of both forms; one step of rechub's AFM model
at 26 x 16 with the switch on and off.

    python profiles/afm.py --resources     # no GPU: VGPR / SGPR / LDS / scratch figures -> profiles/afm/resources.txt
    python profiles/afm.py [--out profiles/afm/table.md] [--quick]

Shapes: B = 4096 and 65 536, F = 26 and 39, D = 16 and 32, A = 25 and 32 (--quick: B = 4096, F = 26 only).  HIP events around
``iters`` steps after a warm-up, median of ``reps`` repetitions, (a) and (b) alternating; a composition that runs out of memory
is recorded as such.  Per sample (fp32) the irreducible traffic of a step is x read by both passes, dx written, out written
and read, dout read: 4 (3 F D + 3 D) bytes; its MFMA work is W p_k forward, again in the backward, dW and W^T dpre:
8 P D A FLOP.  Byte share = those bytes over the step's time over 8 TB/s; MFMA share = those FLOP over the step's time over
157 TFLOP/s (the fp32 matrix peak)."""
import argparse
import os
import re
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HERE = os.path.join(ROOT, "profiles", "afm")
HBM_PEAK, MFMA_PEAK = 8.0e12, 157.0e12


def resources():
    """Compile csrc/rbx_afm.hip alone with -Rpass-analysis=kernel-resource-usage and tabulate what the compiler reports.  The
    forward and backward kernels take their LDS dynamically (sized per shape by the host, at most 64 KiB per workgroup)."""
    from recbox_amd import build
    src = os.path.join(build.CSRC, "rbx_afm.hip")
    cmd = [build._hipcc()] + build.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull]
    text = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, check=True).stdout
    rows, cur = [], None
    for line in text.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|AGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|"
                      r"VGPRs Spill|LDS Size \[bytes/block\]):\s+(\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            k = re.search(r"\d+(afm_\w+?_kernel)(?:ILi(\d+)ELi(\d+)E)?", m.group(2))
            name = m.group(2)
            if k:
                name = k.group(1) + ("<NA=%s, ND=%s>" % (k.group(2), k.group(3)) if k.group(2) else "")
            cur = {"name": name}
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


def _time_ms(fn, iters, reps):
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


def _measure(fn, iters, reps):
    """(median ms, peak MiB above what is allocated before the step) or ("out of memory", None)."""
    try:
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        peak = (torch.cuda.max_memory_allocated() - base) / 2.0 ** 20
        return _time_ms(fn, iters, reps), peak
    except torch.cuda.OutOfMemoryError:
        torch.cuda.empty_cache()
        return "out of memory", None


def pool_rows(quick):
    from recbox_amd import ops
    rows = []
    for B in ((4096,) if quick else (4096, 65536)):
        for F in ((26,) if quick else (26, 39)):
            for D in (16, 32):
                for A in (25, 32):
                    g = torch.Generator().manual_seed(B + F + D + A)
                    x = (torch.randn(B, F, D, generator=g) * 0.5).cuda().requires_grad_()
                    w = (torch.randn(A, D, generator=g) * 0.3).cuda().requires_grad_()
                    h = torch.randn(A, generator=g).cuda().requires_grad_()
                    up = torch.randn(B, D, generator=g).cuda()

                    def step(fn):
                        out, _ = fn(x, w, h)
                        torch.autograd.grad((out * up).sum(), (x, w, h))

                    iters, reps = (10, 7) if B == 4096 else (3, 5)
                    fused = _measure(lambda: step(ops.afm_pool), iters, reps)
                    comp = _measure(lambda: step(ops.afm_pool_torch), iters, reps)
                    P = F * (F - 1) // 2
                    byt, flop = 4.0 * B * (3 * F * D + 3 * D), 8.0 * B * P * D * A
                    rows.append((B, F, D, A, fused, comp, byt / (fused[0] * 1e-3) / HBM_PEAK, flop / (fused[0] * 1e-3) / MFMA_PEAK))
                    print(rows[-1], flush=True)
    return rows


def model_rows():
    from recbox_amd import ops
    from recbox_amd.rechub.basic.features import SparseFeature
    from recbox_amd.rechub.models.ranking import AFM
    torch.manual_seed(0)
    B, F, D = 4096, 26, 16
    feats = [SparseFeature("s%d" % f, vocab_size=1000 + 37 * f, embed_dim=D) for f in range(F)]
    model = AFM(feats, attention_size=25, dropout_prob=0.3).cuda().train()
    opt = torch.optim.SGD(model.parameters(), lr=0.01)
    x = {"s%d" % f: torch.randint(0, 1000 + 37 * f, (B,), device="cuda") for f in range(F)}
    label = torch.randint(0, 2, (B,), device="cuda").float()

    def step():
        opt.zero_grad(set_to_none=True)
        loss = torch.nn.functional.binary_cross_entropy(model(x), label)
        loss.backward()
        opt.step()

    out = []
    for on in (True, False):
        ops.config.afm_fused = on
        out.append(("fused" if on else "composition",) + _measure(step, 10, 7))
    ops.config.afm_fused = True
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.resources:
        text = resources()
        with open(os.path.join(HERE, "resources.txt"), "w") as fh:
            fh.write(text)
        print(text)
        return
    fmt = lambda r: "out of memory" if r[1] is None else "%.3f ms / %.0f MiB" % r   # noqa: E731
    lines = ["| B | F | D | A | fused fwd+bwd / peak | composition fwd+bwd / peak | speed-up | byte share | MFMA share |",
             "|---|---|---|---|---|---|---|---|---|"]
    for B, F, D, A, fused, comp, bs, ms in pool_rows(a.quick):
        sp = "n/a" if comp[1] is None else "%.1fx" % (comp[0] / fused[0])
        lines.append("| %d | %d | %d | %d | %s | %s | %s | %.1f %% | %.1f %% |" % (B, F, D, A, fmt(fused), fmt(comp), sp, 100 * bs,
                                                                               100 * ms))
    lines += ["", "AFM model step (B = 4096, 26 fields x 16, A = 25, SGD):", "", "| interaction | step / peak |", "|---|---|"]
    for name, ms, peak in model_rows():
        lines.append("| %s | %s |" % (name, fmt((ms, peak))))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
