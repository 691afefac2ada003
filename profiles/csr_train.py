"""One training step over ragged bags at BASELINE cfg 3's shape: ``ops.embed_bags`` forward, backward, ``SparseAdam.step``;
one 10 M x 128 table, B = 65 536 bags of 1 .. 50 ids (uniform), MEAN_ID pooling, one hipGraph per step.

    python profiles/csr_train.py [--forms a,b,c] [--rounds 30] [--rows 10000000] [--out FILE]

Forms:
  a  fresh gradients: every backward allocates and zero-fills a [V, D] gradient (``reuse_grad_buffers`` off);
  b  the persistent gradient pool (``reuse_grad_buffers = "all"``), cleared by rbx_embed_csr_rezero in the next forward;
  c  the pool with ``SparseAdam(clear_grads=True)``: the update clears the rows it steps, no re-zero launch.
Every form has its own table, optimiser and captured graph over the same resident batch; after the graphs' warm-up the
forms ALTERNATE inside each round, each replay bracketed by HIP events (median, min, max in microseconds).  On a tree whose
optimiser has no record for a bag-fed table (no rbx_embed_csr_sparse_update) only form a exists, and its step cannot be
captured -- the dense fallback reads on the host: it is then timed eagerly, events around forward + backward + step, and
the report says so.  Kernel times (rezero_rows_kernel, sparse_update_kernel) come from a run of their own under
``rocprofv3 --kernel-trace --stats -- python profiles/csr_train.py --rounds 5``; this script only runs the steps."""
import argparse
import os
import statistics
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from recbox_amd import _lib, ops, optim  # noqa: E402
from recbox_amd.graph import GraphedStep  # noqa: E402

B, D, L = 65536, 128, 50
HAS_BAG_STEP = "rbx_embed_csr_sparse_update" in _lib.SIGNATURES


class Form(object):
    def __init__(self, name, rows, bags, dY):
        self.name = name
        self.pooled, self.clear = name in ("b", "c"), name == "c"
        self.table = torch.nn.Parameter(torch.empty(rows, D, device="cuda").normal_(0, 0.01))
        self.plan = ops.BagPlan([ops.BagSpec("h", D, 0, 0, _lib.POOL_MEAN_ID, rows, mask_id=0, eps=1e-16)])
        self.captured = HAS_BAG_STEP
        kw = {"clear_grads": True} if self.clear else {}
        self.opt = optim.SparseAdam([self.table], lr=1e-3, capturable=self.captured, **kw)

        def fn():
            self.opt.zero_grad()
            ops.embed_bags(self.plan, [bags], [self.table]).backward(dY)
            self.opt.step()

        self.fn = fn
        if self.captured:
            self.step = GraphedStep(fn, warmup=3, reuse_grads="all" if self.pooled else False)
        else:
            for _ in range(3):
                fn()
            self.step = fn
        torch.cuda.synchronize()

    def describe(self):
        how = "one hipGraph" if self.captured else "EAGER (the dense fallback cannot be captured)"
        return {"a": "fresh gradients", "b": "pool + rbx_embed_csr_rezero", "c": "pool + clear_grads"}[self.name] + ", " + how


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--forms", default="a,b,c")
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--rows", type=int, default=10000000)
    ap.add_argument("--out", default="", help="also write the markdown report to this file")
    a = ap.parse_args()
    names = [n for n in a.forms.split(",") if n]
    if not HAS_BAG_STEP:
        names = [n for n in names if n == "a"]
    ops.config.check_ids = False
    gen = torch.Generator().manual_seed(7)
    lengths = torch.randint(1, L + 1, (B,), generator=gen)
    offsets = torch.zeros(B + 1, dtype=torch.int64)
    torch.cumsum(lengths, 0, out=offsets[1:])
    bags = ops.Bags(torch.randint(1, a.rows, (int(offsets[-1]),), generator=gen).cuda(), offsets.cuda())
    dY = torch.randn(B, D, generator=gen).cuda()
    forms = [Form(n, a.rows, bags, dY) for n in names]
    times = dict((f.name, []) for f in forms)
    for _ in range(a.rounds):
        for f in forms:
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            f.step()
            e.record()
            e.synchronize()
            times[f.name].append(s.elapsed_time(e) * 1e3)
    ops.check_deferred_ids()
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL,
                                text=True).stdout.strip() or "working tree"
    except OSError:
        commit = "working tree"
    lines = ["box: %s, torch %s; commit: %s; B = %d, table %d x %d, %d lookups, MEAN_ID, SparseAdam; %d rounds, forms alternating, "
             "HIP events around each step" % (torch.cuda.get_device_name(0), torch.__version__, commit, B, a.rows, D, bags.nnz,
                                              a.rounds), "",
             "| form | step us (min .. max) | sparse-row calls | dense fallbacks |", "|---|---|---|---|"]
    for f in forms:
        t = times[f.name]
        lines.append("| %s: %s | %.1f (%.1f .. %.1f) | %d | %d |" % (f.name, f.describe(), statistics.median(t), min(t), max(t),
                                                                   f.opt.calls["rows"], f.opt.calls["dense"]))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
