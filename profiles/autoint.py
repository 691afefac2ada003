"""AutoInt's interacting layer: forward + backward of one layer through (f) the fused op (ops.field_attn:
csrc/rbx_fieldattn.hip), (a) the reference's call of nn.MultiheadAttention on the [F, B, E] view and (b) the project's own
pieces, ops.linear + ops.attention + ops.linear; same GPU, same process, same data; peak memory of every form; and forward +
backward of the 3-layer recbole.AutoIntInteraction with the switch on and off.

    python profiles/autoint.py --resources     # no GPU: VGPR / LDS / scratch figures -> profiles/autoint/resources.txt
    python profiles/autoint.py [--out profiles/autoint/table.md] [--quick]

Shapes: B = 4096 and 65 536, F = 26 and 39, E = 16 and 32, 2 heads, attention dropout 0 and 0.2 (--quick: B = 4096 only).  HIP
events around ``iters`` steps after a warm-up step, ``reps`` repetitions, the forms alternating; the table gives the median and
the (min - max) of the repetitions; a form that runs out of memory is recorded as such.  Per sample (fp32) the irreducible
traffic of a step is x read by both passes, y written, dy read, dx written: 20 F E bytes; byte share = those bytes over the
step's time over 8 TB/s."""
import argparse
import math
import os
import re
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HERE = os.path.join(ROOT, "profiles", "autoint")
HBM_PEAK = 8.0e12


def resources():
    """Compile csrc/rbx_fieldattn.hip alone with -Rpass-analysis=kernel-resource-usage and tabulate what the compiler reports.
    The forward and backward kernels take their LDS dynamically (sized per shape by the host, at most 160 KiB per workgroup)."""
    from recbox_amd import build
    src = os.path.join(build.CSRC, "rbx_fieldattn.hip")
    cmd = [build._hipcc()] + build.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull]
    text = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, check=True).stdout
    rows, cur = [], None
    for line in text.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|AGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|"
                      r"VGPRs Spill|LDS Size \[bytes/block\]):\s+(\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            k = re.search(r"\d+(fieldattn_\w+?_kernel)(?:IL([ib])(\d+)E(?:Lb(\d+)E)?E)?", m.group(2))
            name = m.group(2)
            if k:
                name = k.group(1)
                if k.group(2) == "i":
                    name += "<NE=%s, DROP=%s>" % (k.group(3), k.group(4))
                elif k.group(2) == "b":
                    name += "<DROP=%s>" % k.group(3)
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


def _times_ms(fn, iters, reps):
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
    return sorted(times)


def _measure(fn, iters, reps):
    """(median ms, min ms, max ms, peak MiB above what is allocated before the step) or None when out of memory."""
    try:
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        peak = (torch.cuda.max_memory_allocated() - base) / 2.0 ** 20
        t = _times_ms(fn, iters, reps)
        return t[len(t) // 2], t[0], t[-1], peak
    except torch.cuda.OutOfMemoryError:
        torch.cuda.empty_cache()
        return None


def _pieces(x, in_w, in_b, out_w, out_b, heads, p):
    """(b): the layer from ops.linear, ops.attention, ops.linear."""
    from recbox_amd import ops
    B, F, E = x.shape
    dh = E // heads
    qkv = ops.linear(x.reshape(B * F, E), in_w, in_b).view(B, F, 3, heads, dh)
    q, k, v = (qkv[:, :, i].transpose(1, 2) for i in range(3))
    o, _ = ops.attention(q, k, v, scale=1.0 / math.sqrt(dh), dropout_p=p)
    return ops.linear(o.transpose(1, 2).reshape(B * F, E), out_w, out_b).view(B, F, E)


def layer_rows(quick):
    from recbox_amd import ops
    rows = []
    for B in ((4096,) if quick else (4096, 65536)):
        for F in (26, 39):
            for E in (16, 32):
                for p in (0.0, 0.2):
                    torch.manual_seed(B + F + E)
                    mha = torch.nn.MultiheadAttention(E, 2, dropout=p).cuda().train()
                    params = (mha.in_proj_weight, mha.in_proj_bias, mha.out_proj.weight, mha.out_proj.bias)
                    fbe = torch.randn(F, B, E, device="cuda").requires_grad_()
                    up = torch.randn(B, F, E, device="cuda")

                    def step(form):
                        x = fbe.transpose(0, 1)
                        if form == "f":
                            y = ops.field_attn(x, *params, 2, dropout_p=p)[0]
                        elif form == "a":
                            y = mha(fbe, fbe, fbe)[0].transpose(0, 1)
                        else:
                            y = _pieces(x, *params, 2, p)
                        torch.autograd.grad((y * up).sum(), (fbe,) + params)

                    iters, reps = (10, 7) if B == 4096 else (3, 5)
                    res = [_measure(lambda form=form: step(form), iters, reps) for form in ("f", "a", "b")]
                    rows.append((B, F, E, p, res, 20.0 * B * F * E / (res[0][0] * 1e-3) / HBM_PEAK))
                    print(rows[-1], flush=True)
                    del mha, fbe, up
                    torch.cuda.empty_cache()
    return rows


def interaction_rows(quick):
    from recbox_amd import ops
    from recbox_amd.recbole import AutoIntInteraction
    out = []
    for B in ((4096,) if quick else (4096, 65536)):
        torch.manual_seed(0)
        F, D = 39, 16
        m = AutoIntInteraction(F, D, 16, 3, 2, [128, 128], [0.2, 0.2, 0.2], True).cuda().train()
        x = torch.randn(B, F, D, device="cuda").requires_grad_()

        def step():
            torch.autograd.grad(m(x).sum(), [x] + list(m.parameters()))

        for on in (True, False):
            ops.config.field_attn_fused = on
            out.append((B, "fused" if on else "composition", _measure(step, 5, 5)))
            print(out[-1], flush=True)
        ops.config.field_attn_fused = True
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
    fmt = lambda r: "out of memory" if r is None else "%.3f (%.3f - %.3f) ms / %.0f MiB" % r   # noqa: E731
    lines = ["| B | F | E | p | fused fwd+bwd / peak | (a) nn.MultiheadAttention | (b) linear + attention + linear | vs (a) | vs (b) "
             "| byte share |", "|---|---|---|---|---|---|---|---|---|---|"]
    for B, F, E, p, res, share in layer_rows(a.quick):
        sp = ["n/a" if r is None else "%.2fx" % (r[0] / res[0][0]) for r in res[1:]]
        lines.append("| %d | %d | %d | %.1f | %s | %s | %s | %s | %s | %.1f %% |" % (B, F, E, p, fmt(res[0]), fmt(res[1]), fmt(res[2]),
                                                                                 sp[0], sp[1], 100 * share))
    lines += ["", "AutoIntInteraction forward + backward (39 fields x 16, A = 16, 3 layers, 2 heads, MLP 128-128, dropout 0.2, "
              "residual):", "", "| B | layers | step / peak |", "|---|---|---|"]
    for B, name, r in interaction_rows(a.quick):
        lines.append("| %d | %s | %s |" % (B, name, fmt(r)))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
