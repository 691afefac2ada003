"""Time ops.search_ip (rbx_search_ip: no score matrix) against the matrix path topk(linear(U, V), k) run in the block size
evaluate_metrics gives it (min(1000, 2^28 // n_items) users per block), HIP events on the launch stream.

    python profiles/search_ip.py [--out FILE] [--iters N]

Prints one markdown table row per shape: the median of N timed calls after one warm-up call, per 1000 users."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from recbox_amd import ops  # noqa: E402

SHAPES = [(1000, 1 << 18, 128, 500), (1000, 1 << 20, 128, 500), (1000, 10 ** 7, 128, 500), (1000, 1 << 20, 32, 500)]


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=5)
    a = ap.parse_args()
    lines = ["| users | n_items | dim | k | parent block | parent ms (median, min-max) | fused ms (median, min-max) | fused rows | speed-up |",
             "|---|---|---|---|---|---|---|---|---|"]
    g = torch.Generator().manual_seed(0)
    for users, n, dim, k in SHAPES:
        U = (torch.rand((users, dim), generator=g) - 0.5).cuda()
        V = torch.empty((n, dim), device="cuda").uniform_(-0.5, 0.5)
        block = max(1, min(1000, (1 << 28) // n))

        def parent():
            for i in range(0, users, block):
                ops.topk(ops.linear(U[i:i + block], V), k)

        def fused():
            ops.search_ip(U, V, k)

        f = timed(fused, a.iters)
        fused_rows = ops.search_ip_stats["fused_rows"]
        p = timed(parent, a.iters)
        line = "| %d | %d | %d | %d | %d | %.2f (%.2f-%.2f) | %.2f (%.2f-%.2f) | %d | %.2fx |" % (
            users, n, dim, k, block, p[0], p[1], p[2], f[0], f[1], f[2], fused_rows, p[0] / f[0])
        print(line, flush=True)
        lines.append(line)
        del U, V
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
