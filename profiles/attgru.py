"""Forward + backward of ops.att_gru (csrc/rbx_gru.hip) against the step-loop composition ops.att_gru_torch, same process,
same inputs, alternating:

    python profiles/attgru.py [--out profiles/attgru/table.md] [--quick]

Both cells at L = 50, I = H = 16 / 64 / 128, B = 4096 and 65 536, plus one DIEN-like shape (B = 512, L = 20, H = 32).  Per
shape and implementation: 3 warm-up steps, then ``reps`` timed steps between device events in rounds that alternate the two
implementations (the median round is reported, the spread is the min .. max of the rounds); peak memory is
torch.cuda.max_memory_allocated over one step after a reset.  Lengths uniform in 1 .. L, scores ~ U(0, 1).  Needs a GPU: there
is no fallback."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(4096, 50, 16), (4096, 50, 64), (4096, 50, 128), (65536, 50, 16), (65536, 50, 64), (65536, 50, 128), (512, 20, 32)]


def make(B, L, H, seed=0):
    g = torch.Generator().manual_seed(seed)
    bound = 1.0 / H ** 0.5

    def uni(*shape):
        return ((torch.rand(*shape, generator=g) * 2 - 1) * bound).cuda().requires_grad_(True)
    return {"x": torch.randn(B, L, H, generator=g).cuda().requires_grad_(True),
            "att": torch.rand(B, L, generator=g).cuda().requires_grad_(True),
            "p": [uni(3 * H, H), uni(3 * H, H), uni(3 * H), uni(3 * H)],
            "lengths": torch.randint(1, L + 1, (B,), generator=g).cuda(),
            "up": (torch.randn(B, H, generator=g) / B ** 0.5).cuda()}


def step(fn, d, cell):
    for t in [d["x"], d["att"]] + d["p"]:
        t.grad = None
    out, hn = fn(d["x"], d["att"], d["p"][0], d["p"][1], d["p"][2], d["p"][3], None, d["lengths"], cell)
    (hn * d["up"]).sum().backward()                          # DIEN reads the final state alone


def timed(fn, d, cell, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        step(fn, d, cell)
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / reps


def peak(fn, d, cell):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    step(fn, d, cell)
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="fewer rounds and repetitions (a rehearsal, not a measurement)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "profiles/attgru.py needs a GPU"
    from recbox_amd import ops
    lines = ["| cell | B | L | H | fused ms (min .. max) | composition ms (min .. max) | ratio | fused peak MiB | composition peak MiB |",
             "|---|---|---|---|---|---|---|---|---|"]
    for cell in ("AGRU", "AUGRU"):
        for B, L, H in SHAPES:
            d = make(B, L, H)
            big = B * L * H >= 2 ** 26
            rounds = 2 if args.quick else 5
            reps_f = 2 if args.quick else (5 if big else 20)
            reps_c = 1 if args.quick else (2 if big else 5)
            for fn in (ops.att_gru, ops.att_gru_torch):
                for _ in range(3):
                    step(fn, d, cell)
            torch.cuda.synchronize()
            tf, tc = [], []
            for _ in range(rounds):
                tf.append(timed(ops.att_gru, d, cell, reps_f))
                tc.append(timed(ops.att_gru_torch, d, cell, reps_c))
            mf, mc = statistics.median(tf), statistics.median(tc)
            line = "| %s | %d | %d | %d | %.3f (%.3f .. %.3f) | %.3f (%.3f .. %.3f) | %.1f x | %.0f | %.0f |" % (
                cell, B, L, H, mf, min(tf), max(tf), mc, min(tc), max(tc), mc / mf, peak(ops.att_gru, d, cell),
                peak(ops.att_gru_torch, d, cell))
            print(line, flush=True)
            lines.append(line)
            del d
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
