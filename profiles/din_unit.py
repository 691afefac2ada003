"""Time DIN's activation unit, forward + backward, with ops.config.din_fused on (rbx_din_*: no [B, L, 4E] tensor) and off
(the composition it replaces: concatenate, GEMM, mask / softmax / weighted sum by ATen), HIP events on the launch stream,
the two alternating in one process.

    python profiles/din_unit.py [--out FILE] [--iters N] [--rounds R]

Prints one markdown table row per shape: median and min-max over R rounds of the mean of N steps, and what share of the
byte bound of the two pairs kernels' forward (read h, write y) and of the whole fused step the times come to."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from recbox_amd import ops  # noqa: E402
from recbox_amd.ranking.pytorch.layers.attentions import DIN_Attention  # noqa: E402
from recbox_amd.rechub.models.ranking import ActivationUnit  # noqa: E402

HBM_BYTES_PER_S = 8.0e12          # MI355X peak
# name, B, L, E, module factory, takes a mask
SHAPES = [
    ("ranking relu [64, 32]", 4096, 50, 64, lambda: DIN_Attention(64, [64, 32], "ReLU", use_softmax=True), True),
    ("ranking dice [64, 32]", 4096, 50, 64, lambda: DIN_Attention(64, [64, 32], "Dice", use_softmax=True), True),
    ("wide relu [64, 32]", 4096, 50, 128, lambda: DIN_Attention(128, [64, 32], "ReLU", use_softmax=True), True),
    ("narrow-n relu [16]", 4096, 50, 64, lambda: DIN_Attention(64, [16], "ReLU", use_softmax=True), True),
    ("short-L relu [64, 32]", 4096, 10, 64, lambda: DIN_Attention(64, [64, 32], "ReLU", use_softmax=True), True),
    ("E = 32 relu [64, 32]", 4096, 50, 32, lambda: DIN_Attention(32, [64, 32], "ReLU", use_softmax=True), True),
    ("rechub dice [36]", 4096, 50, 16, lambda: ActivationUnit(16, dims=[36], activation="dice", use_softmax=True), False),
]


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=200)          # a round of 200 steps is 0.2-0.4 s
    ap.add_argument("--only", default=None, help="time the one shape of this name")
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    lines = ["| unit | B | L | E | n | composition ms (median, min-max) | fused ms (median, min-max) | speed-up | "
             "pairs fwd us | h + y bound us | share |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    g = torch.Generator().manual_seed(0)
    for name, B, L, E, make, masked in SHAPES:
        if a.only and a.only != name:
            continue
        net = make().cuda().train()
        t = torch.randn(B, E, generator=g).cuda().requires_grad_()
        h = torch.randn(B, L, E, generator=g).cuda().requires_grad_()
        mask = (torch.rand(B, L, generator=g) < 0.7).float().cuda()

        def step():
            for p in list(net.parameters()) + [t, h]:
                p.grad = None
            out = net(t, h, mask) if masked else net(h, t)
            out.sum().backward()

        ops.config.din_min_dim = 4                     # time the fused path at every width, whatever the default routes
        times = {True: [], False: []}
        for fused in (True, False):                    # warm both paths
            ops.config.din_fused = fused
            step(), step()
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for fused in (True, False):
                ops.config.din_fused = fused
                times[fused].append(timed(step, a.iters))
        ops.config.din_fused = True
        first = (net.attention_layer.mlp if masked else net.attention.mlp)[0]
        n = first.out_features
        with torch.no_grad():
            pf = [timed(lambda: ops.din_scores(h, t, first.weight, first.bias), a.iters) for _ in range(a.rounds)]
        bound = (B * L * E + B * L * n) * 4 / HBM_BYTES_PER_S * 1e6
        f, c = times[True], times[False]
        line = "| %s | %d | %d | %d | %d | %.3f (%.3f-%.3f) | %.3f (%.3f-%.3f) | %.2fx | %.1f | %.1f | %.0f %% |" % (
            name, B, L, E, n, statistics.median(c), min(c), max(c), statistics.median(f), min(f), max(f),
            statistics.median(c) / statistics.median(f), statistics.median(pf) * 1e3, bound,
            100.0 * bound / (statistics.median(pf) * 1e3))
        print(line, flush=True)
        lines.append(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
