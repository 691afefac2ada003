"""Field-aware FM: ops.ffm_cross (csrc/rbx_ffm.hip) against the two ways of composing it, forward + backward.

    python profiles/ffm.py [--batches 4096 65536] [--fields 26 39] [--dims 4 8 16] [--out profiles/ffm/times.txt]

(a) the vectorised ATen composition the models fall back to: F.embedding of x * F + arange(F) per field into
    [B, F, F, D], one indexed multiply x[:, I, J] * x[:, J, I];
(b) the reference's literal loop: P sliced multiplies and a stack (third_party/rechub/basic/layers.py:671-677).
Same GPU, same data, HIP events around `iters` steps after a warm-up, median of `reps` repetitions.  Also each fused
kernel's share of its byte bound at `--hbm-gbs`: forward F(F-1) 4D bytes read + P 4D written per sample, backward the same
rows plus dout read twice (kernel times from HIP events around the C-ABI calls, ops.kernel_timer)."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--fields", type=int, nargs="+", default=[26, 39])
    ap.add_argument("--dims", type=int, nargs="+", default=[4, 8, 16])
    ap.add_argument("--blocks", type=int, default=1000, help="ids per table (uniform)")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0)
    ap.add_argument("--loop-max-bytes", type=float, default=6e9, help="skip baseline (b) when [B, F, F, D] x 4 exceeds it")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from recbox_amd import ops
    from recbox_amd.rechub.basic.layers import FFM
    ops.config.check_ids = False
    lines = ["# B F D | fused ms | (a) indexed ms | (b) loop ms | a/fused b/fused | fwd kernel us (share of byte bound) | "
             "bwd reduce us (share)"]
    for B in a.batches:
        for F in a.fields:
            for D in a.dims:
                g = torch.Generator().manual_seed(1)
                tables = [(torch.randn(a.blocks * F, D, generator=g) * 0.1).cuda().requires_grad_(True) for _ in range(F)]
                ids = [torch.randint(0, a.blocks, (B,), generator=g).cuda() for _ in range(F)]
                P = F * (F - 1) // 2
                r = torch.randn(B, P, D, device="cuda")
                off = torch.arange(F, device="cuda")
                ffm = FFM(F, reduce_sum=False).cuda()

                def gather():
                    return torch.stack([torch.nn.functional.embedding(x.reshape(-1, 1) * F + off, t)
                                        for t, x in zip(tables, ids)], dim=1)

                def fused():
                    torch.autograd.grad(ops.ffm_cross(tables, ids), tables, r)

                def indexed():
                    torch.autograd.grad(ffm(gather()), tables, r)

                def loop():
                    x = gather()
                    out = torch.stack([x[:, i, j] * x[:, j, i] for i in range(F - 1) for j in range(i + 1, F)], dim=1)
                    torch.autograd.grad(out, tables, r)

                t_f = _time(fused, a.iters, a.reps)
                t_a = _time(indexed, a.iters, a.reps)
                t_b = _time(loop, a.iters, a.reps) if B * F * F * D * 16.0 <= a.loop_max_bytes else float("nan")
                kern = {}
                for tag in ("ffm_fwd", "ffm_bwd"):
                    ops.kernel_timer = ops.KernelTimer(lambda meta, tag=tag: meta[0] == tag)
                    for _ in range(a.iters):
                        fused()
                    torch.cuda.synchronize()
                    kern[tag] = ops.kernel_timer.mean_ms() * 1e3
                    ops.kernel_timer = None
                fwd_bytes = B * (F * (F - 1) * 4 * D + P * 4 * D)
                bwd_bytes = B * (F * (F - 1) * 4 * D + 2 * P * 4 * D + F * (F - 1) * 4 * D)
                share = lambda us, nbytes: nbytes / (a.hbm_gbs * 1e3) / us if us else float("nan")   # noqa: E731
                lines.append("%6d %2d %3d | %8.3f | %8.3f | %8.3f | %5.2fx %5.2fx | %8.1f (%4.2f) | %8.1f (%4.2f)"
                             % (B, F, D, t_f, t_a, t_b, t_a / t_f, t_b / t_f, kern["ffm_fwd"],
                                share(kern["ffm_fwd"], fwd_bytes), kern["ffm_bwd"], share(kern["ffm_bwd"], bwd_bytes)))
                print(lines[-1], flush=True)
                del tables, ids, r
                torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
