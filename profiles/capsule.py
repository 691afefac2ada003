"""Multi-interest routing, bilinear form (ComirecDR): ops.capsule_bilinear_route (csrc/rbx_capsule.hip) against the two ways
of composing it, forward and forward + backward.

    python profiles/capsule.py [--batch 8192] [--seq-len 50] [--interests 4] [--dim 64] [--out profiles/capsule/times.txt]

(a) the einsum composition the mirror falls back to (ops.capsule_bilinear_torch + ops.capsule_route_torch): no
    [B, L, K D, D] product, about 15 ATen kernels per routing iteration;
(b) the reference's literal expression, torch.sum(w * x.unsqueeze(2), dim=3) (third_party/rechub/basic/layers.py:595-596)
    followed by the same routing loop, at the largest batch (a power of two, at most --batch) for which four copies of its
    [B, L, K D, D] product fit in free memory; the batch used is printed.
Same GPU, same process, same data, HIP events around `iters` steps after a warm-up, median of `reps` repetitions.  Then each
kernel alone (HIP events around the C-ABI calls, ops.kernel_timer) with the bytes it must move, its FLOPs, and the share of
the larger of its two bounds at --hbm-gbs / --f32-tflops."""
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
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--seq-len", type=int, default=50)
    ap.add_argument("--interests", type=int, default=4)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0)
    ap.add_argument("--f32-tflops", type=float, default=157.3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from recbox_amd import ops
    B, L, K, D = a.batch, a.seq_len, a.interests, a.dim
    N = K * D
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, L, D, generator=g).cuda().requires_grad_(True)
    w = (torch.randn(1, L, N, D, generator=g) / D ** 0.5).cuda().requires_grad_(True)
    lengths = torch.randint(0, L + 1, (B,), generator=g)
    mask = (torch.arange(L).unsqueeze(0) < lengths.unsqueeze(1)).long().cuda()
    r = torch.randn(B, K, D, generator=g).cuda()

    def fused(xx=x, mm=mask):
        return ops.capsule_bilinear_route(xx, w, mm, K)

    def einsum(xx=x, mm=mask):
        return ops.capsule_route_torch(ops.capsule_bilinear_torch(xx, w), mm, K)

    def literal(xx, mm):
        hat = torch.sum(w[:, :L, :, :] * torch.unsqueeze(xx, dim=2), dim=3)
        return ops.capsule_route_torch(hat, mm, K)

    def fwd(fn, *args):
        def run():
            with torch.no_grad():
                fn(*args)
        return run

    def both(fn, xx, rr, *args):
        return lambda: torch.autograd.grad(fn(xx, *args), [xx, w], rr)

    lines = ["# B=%d L=%d K=%d D=%d: [B, L, K D, D] would be %.1f MB per sample, %.1f GB in all"
             % (B, L, K, D, L * N * D * 4 / 1e6, B * L * N * D * 4.0 / 1e9)]
    t = {"fused fwd": _time(fwd(fused), a.iters, a.reps), "fused fwd+bwd": _time(both(fused, x, r, mask), a.iters, a.reps),
         "einsum fwd": _time(fwd(einsum), a.iters, a.reps), "einsum fwd+bwd": _time(both(einsum, x, r, mask), a.iters, a.reps)}
    lines.append("fused        fwd %8.3f ms   fwd+bwd %8.3f ms" % (t["fused fwd"], t["fused fwd+bwd"]))
    lines.append("(a) einsum   fwd %8.3f ms   fwd+bwd %8.3f ms   %.2fx / %.2fx the fused time"
                 % (t["einsum fwd"], t["einsum fwd+bwd"], t["einsum fwd"] / t["fused fwd"],
                    t["einsum fwd+bwd"] / t["fused fwd+bwd"]))
    print("\n".join(lines), flush=True)

    free, _ = torch.cuda.mem_get_info()
    Bl = 1
    while Bl * 2 <= B and 4.0 * (Bl * 2) * L * N * D * 4 <= 0.8 * free:
        Bl *= 2
    xl, ml, rl = x[:Bl].detach().clone().requires_grad_(True), mask[:Bl].clone(), r[:Bl].clone()
    tl = (_time(fwd(literal, xl, ml), 3, 3), _time(both(literal, xl, rl, ml), 3, 3))
    tf = (_time(fwd(fused, xl, ml), a.iters, a.reps), _time(both(fused, xl, rl, ml), a.iters, a.reps))
    lines.append("(b) literal at B=%d (product %.2f GB; four copies fit in %.0f GB free): fwd %8.3f ms   fwd+bwd %8.3f ms; fused "
                 "at that B: %8.3f / %8.3f ms   %.1fx / %.1fx" % (Bl, Bl * L * N * D * 4.0 / 1e9, free / 1e9, tl[0], tl[1],
                                                                 tf[0], tf[1], tl[0] / tf[0], tl[1] / tf[1]))
    print(lines[-1], flush=True)
    del xl, ml, rl
    torch.cuda.empty_cache()

    splits = (B + ops.CAPSULE_DW_SPLIT - 1) // ops.CAPSULE_DW_SPLIT
    gemm = 2.0 * B * L * N * D
    work = {    # kernel: (bytes it must move, FLOPs)
        "capsule_hat": (4.0 * (B * L * D + L * N * D + B * L * N), gemm),
        "capsule_route_fwd": (4.0 * (B * L * N + 2 * B * L + 2 * B * K * D + B * K * L), 3 * 4.0 * B * K * L * D),
        "capsule_route_bwd": (4.0 * 3 * B * K * D, 0.0),
        "capsule_bilinear_dx": (4.0 * (B * N + B * K * L + L * N * D + B * L * D), gemm),
        "capsule_bilinear_dw": (4.0 * (B * L * D + B * N + B * K * L + (2 * splits if splits > 1 else 0) * L * N * D
                                       + L * N * D), gemm),
    }
    lines.append("# kernel | us | MB moved | GFLOP | share of its bound (which)")
    step = both(fused, x, r, mask)
    for tag, (nbytes, flops) in work.items():
        ops.kernel_timer = ops.KernelTimer(lambda meta, tag=tag: meta[0] == tag)
        for _ in range(a.iters):
            step()
        torch.cuda.synchronize()
        us = ops.kernel_timer.mean_ms() * 1e3
        ops.kernel_timer = None
        t_mem, t_mm = nbytes / (a.hbm_gbs * 1e3), flops / (a.f32_tflops * 1e6)
        lines.append("%-20s | %8.1f | %8.1f | %7.2f | %4.2f (%s)" % (tag, us, nbytes / 1e6, flops / 1e9,
                                                                    max(t_mem, t_mm) / us if us else float("nan"),
                                                                    "HBM" if t_mem >= t_mm else "fp32 MFMA"))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
