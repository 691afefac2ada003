"""GRU layers of the session-based models: forward + backward of (a) the fused op (ops.gru: csrc/rbx_gru.hip), (b) the
step-loop composition it replaces (ops.gru_torch: ops.linear per step + ATen gates) and (c) torch.nn.GRU on the same device
(the vendor library's RNN; for information only, it is not on this project's path).

    python profiles/gru.py --resources           # no GPU: the kernels' VGPR / LDS / scratch figures -> profiles/gru/resources.txt
    python profiles/gru.py [--out profiles/gru/INDEX.md] [--quick]

Shapes: GRU4Rec's form (2 bias-free layers, I = H, only h_n used) at B = 4096 and 65 536, L = 50, H = 16 / 64 / 128; NARM's
form (1 layer with biases, B = 512, L = 20, I = 50, H = 100, lengths uniform in 1 .. L, out and h_n used).  Same GPU, same
process, same data; HIP events around `iters` steps after a warm-up, median of `reps` repetitions.  (c) runs NARM's form without
lengths: packing needs a host copy of them."""
import argparse
import os
import re
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HERE = os.path.join(ROOT, "profiles", "gru")
CELLS = ("AGRU", "AUGRU", "GRU")                 # csrc/rbx_gru.hip's GruCell


def resources():
    """Compile csrc/rbx_gru.hip alone with -Rpass-analysis=kernel-resource-usage and tabulate what the compiler reports."""
    from recbox_amd import build
    src = os.path.join(build.CSRC, "rbx_gru.hip")
    cmd = [build._hipcc()] + build.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull]
    text = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, check=True).stdout
    rows, cur = [], None
    for line in text.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|AGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|"
                      r"VGPRs Spill|LDS Size \[bytes/block\]):\s+(\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            k = re.search(r"gru_(fwd|bwd)_kernelILi(\d+)ELi(\d+)E", m.group(2))
            cur = {"name": "gru_%s_kernel<%s, %s>" % (k.group(1), k.group(2), CELLS[int(k.group(3))]) if k else m.group(2)}
            rows.append(cur)
        elif cur is not None:
            cur[m.group(1)] = m.group(2)
    rows.sort(key=lambda r: r["name"].split(",")[-1])          # cell by cell; within one, the compiler's order
    lines = ["| kernel (k-steps laid out: H <= 4 x; cell) | VGPRs | AGPRs | SGPRs | scratch B/lane | VGPR spills | LDS B/block | waves/SIMD |",
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


def _case(B, L, I, H, layers, bias, use_out, with_lengths, iters, reps):
    from recbox_amd import ops
    g = torch.Generator().manual_seed(1)
    bound = 1.0 / H ** 0.5
    x = torch.randn(B, L, I, generator=g).cuda().requires_grad_(True)
    ref = torch.nn.GRU(I, H, num_layers=layers, bias=bias, batch_first=True).cuda()
    params = [[getattr(ref, "%s_l%d" % (n, k), None) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
              for k in range(layers)]
    for p in ref.parameters():
        with torch.no_grad():
            p.uniform_(-bound, bound)
    lengths = torch.randint(1, L + 1, (B,), generator=g).cuda() if with_lengths else None
    up_h = torch.randn(B, H, generator=g).cuda()
    up_o = torch.randn(B, L, H, generator=g).cuda() if use_out else None
    leaves = [x] + [p for layer in params for p in layer if p is not None]

    def stack(fn):
        def run():
            cur = x
            for layer in params:
                cur, h = fn(cur, layer[0], layer[1], layer[2], layer[3], None, lengths)
            loss = (h * up_h).sum()
            if up_o is not None:
                loss = loss + (cur * up_o).sum()
            torch.autograd.grad(loss, leaves)
        return run

    def vendor():
        out, hn = ref(x)
        loss = (hn[-1] * up_h).sum()
        if up_o is not None:
            loss = loss + (out * up_o).sum()
        torch.autograd.grad(loss, leaves)

    res = {}
    for tag, fn in (("fused", stack(ops.gru)), ("loop", stack(ops.gru_torch)), ("torch.nn.GRU", vendor)):
        try:
            res[tag] = _time(fn, iters, reps)
        except torch.cuda.OutOfMemoryError:
            res[tag] = None
        except RuntimeError as exc:                      # the vendor RNN refuses some sizes (miopenStatusBadParm)
            if tag != "torch.nn.GRU":
                raise
            res[tag] = None
            print("torch.nn.GRU at B=%d H=%d: %s" % (B, H, str(exc).splitlines()[0]), flush=True)
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
    cases = []
    for B in ([4096] if a.quick else [4096, 65536]):
        for H in (16, 64, 128):
            cases.append(("GRU4Rec", B, 50, H, H, 2, False, False, False))
    cases.append(("NARM", 512, 20, 50, 100, 1, True, True, True))
    lines = ["# GRU: fused recurrence (csrc/rbx_gru.hip) against the step loop, forward + backward", "",
             "Written by `python profiles/gru.py` on %s; median of %d x %d steps, HIP events."
             % (torch.cuda.get_device_name(0), a.reps, a.iters), "",
             "| form | B | L | I | H | layers | (a) fused ms | (b) step loop ms | (b) / (a) | (c) torch.nn.GRU ms | (c) / (a) |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]

    def ms(v):
        return "%.3f" % v if v is not None else "not measured (out of memory, or refused by the library)"

    def ratio(v, base):
        return "%.2f x" % (v / base) if (v is not None and base) else "-"
    for form, B, L, I, H, layers, bias, use_out, with_len in cases:
        big = B > 8192
        r = _case(B, L, I, H, layers, bias, use_out, with_len, 2 if big else a.iters, 2 if big else a.reps)
        lines.append("| %s | %d | %d | %d | %d | %d | %s | %s | %s | %s | %s |"
                     % (form, B, L, I, H, layers, ms(r["fused"]), ms(r["loop"]), ratio(r["loop"], r["fused"]),
                        ms(r["torch.nn.GRU"]), ratio(r["torch.nn.GRU"], r["fused"])))
        print(lines[-1], flush=True)
    lines += ["", "## Compiler resource figures (hipcc -Rpass-analysis=kernel-resource-usage, gfx950)", ""]
    lines.append(open(res_path).read() if os.path.exists(res_path) else resources())
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
