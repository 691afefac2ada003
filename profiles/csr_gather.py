"""Ragged (CSR) gather-pool against the padded lookup at BASELINE cfg 3's shape: B = 65 536 samples, one 10 M x 128 table,
MEAN_ID pooling.  Times the C-ABI calls themselves (forward, id sort, backward with accumulate = 1 into a persistent
gradient, so that no zero fill is inside the bracket) with HIP events on torch's current stream: 3 warm-up rounds, then
``--repeats`` rounds in which the variants of a case ALTERNATE in one process; median, min and max per call in microseconds.

    python profiles/csr_gather.py [--repeats 20] [--rows 10000000] [--out FILE]

Cases: (1) every bag 50 ids = the padded L = 50 call's lookups; (2) lengths uniform in 1 .. 50 against the same ids padded
to 50; (3) skewed lengths (bags of 1 .. 9 ids, 0.1 % of them 1 000 .. 5 000) against the same nnz spread evenly, the skewed
batch with the long-bag form off (threshold 0: a lane group per bag) and on (``--threshold``, default the one in force)
alternating; (4) case 2's bags under SUM_ID with and without per-sample weights, and the weight-gradient call; (5) case
2's bags under SUM_ID against POOL_MAX (rbx_embed_csr_fwd_max, the position-valued sort, rbx_embed_csr_bwd_max), and the
ATen routes to a max over the same ids.  Every CSR variant calls what ``ops.embed_bags`` calls: the ``_long`` entry points
with the threshold, the plain ones at 0.  ``--cases 5`` runs a subset."""
import argparse
import os
import statistics
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from recbox_amd import _embed_host as host  # noqa: E402
from recbox_amd import _lib, ops  # noqa: E402
from recbox_amd._lib import lib  # noqa: E402

B, D, L = 65536, 128, 50


def bracket(fns, repeats):
    """[(median, min, max) in us] of every callable, the callables alternating inside each round."""
    for _ in range(3):
        for f in fns:
            f()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(repeats):
        for t, f in zip(times, fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            t.append(a.elapsed_time(b) * 1e3)
    return [(statistics.median(t), min(t), max(t)) for t in times]


class Padded(object):
    def __init__(self, emb, grad, ids):
        self.plan = host.Plan([host.Lookup("h", _lib.FIELD_CATEGORICAL, emb, D, pool=_lib.POOL_MEAN_ID, seq_len=ids.shape[1],
                                           mask_id=0, eps=1e-16)]).plan
        self.ids, self.w, self.g = ids, emb.weight, grad
        self.out = torch.empty(B, D, device="cuda")
        self.scale = torch.empty(1, B, device="cuda")
        self.plan.bind_inputs([ids])
        self.plan.bind_params([self.w], [self.g])
        self.nbytes = lib.rbx_embed_bwd_workspace_size(self.plan.arr, 1, B)
        self.ws = torch.empty(self.nbytes, dtype=torch.uint8, device="cuda")
        self.lookups = ids.numel()

    def fwd(self):
        _lib.check(lib.rbx_embed_fwd(self.plan.arr, 1, B, self.out.data_ptr(), D, self.scale.data_ptr(), None, ops._stream()))

    def sort(self):
        _lib.check(lib.rbx_embed_sort(self.plan.arr, 1, B, self.ws.data_ptr(), self.nbytes, None, ops._stream()))

    def bwd(self):
        _lib.check(lib.rbx_embed_bwd(self.plan.arr, 1, B, self.out.data_ptr(), D, self.scale.data_ptr(), 1, self.ws.data_ptr(),
                                     self.nbytes, ops._stream()))


def long_workspace(plan, threshold):
    nbytes = lib.rbx_embed_csr_fwd_long_workspace_size(plan.arr, plan.n, B, threshold)
    return torch.empty(max(nbytes, 1), dtype=torch.uint8, device="cuda"), nbytes


def long_counts(ws):
    """(bags that took the long form, segments) of the last ``_long`` call over this workspace."""
    words = ws[:8].view(torch.int32).tolist()
    return words[_lib.CSR_WS_LONG_BAGS], words[_lib.CSR_WS_SEGMENTS]


class Ragged(object):
    def __init__(self, emb, grad, bags, threshold=None):
        self.threshold = ops.bag_long_threshold() if threshold is None else threshold
        self.plan = ops.BagPlan([ops.BagSpec("h", D, 0, 0, _lib.POOL_MEAN_ID, emb.num_embeddings, mask_id=0, eps=1e-16)])
        self.bags, self.w, self.g = bags, emb.weight, grad
        self.out = torch.empty(B, D, device="cuda")
        self.scale = torch.empty(1, B, device="cuda")
        self.plan.bind_inputs([bags])
        self.plan.bind_params([self.w], [self.g])
        self.nbytes = lib.rbx_embed_csr_bwd_workspace_size(self.plan.arr, 1, B)
        self.ws = torch.empty(self.nbytes, dtype=torch.uint8, device="cuda")
        self.lookups = bags.nnz
        self.lws, self.lbytes = long_workspace(self.plan, self.threshold)

    def fwd(self):
        if self.threshold > 0:
            _lib.check(lib.rbx_embed_csr_fwd_long(self.plan.arr, 1, B, self.threshold, self.out.data_ptr(), D, self.scale.data_ptr(),
                                                  self.lws.data_ptr(), self.lbytes, None, ops._stream()))
        else:
            _lib.check(lib.rbx_embed_csr_fwd(self.plan.arr, 1, B, self.out.data_ptr(), D, self.scale.data_ptr(), None,
                                             ops._stream()))

    def sort(self):
        _lib.check(lib.rbx_embed_csr_sort(self.plan.arr, 1, B, self.ws.data_ptr(), self.nbytes, None, ops._stream()))

    def bwd(self):
        _lib.check(lib.rbx_embed_csr_bwd(self.plan.arr, 1, B, self.out.data_ptr(), D, self.scale.data_ptr(), 1,
                                         self.ws.data_ptr(), self.nbytes, ops._stream()))


class Weighted(object):
    """Case 2's bags under SUM_ID, without and with per-sample weights (the ``_weighted`` entry points and the
    weight-gradient kernel)."""

    def __init__(self, emb, grad, bags, weighted):
        self.plan = ops.BagPlan([ops.BagSpec("h", D, 0, 0, _lib.POOL_SUM_ID, emb.num_embeddings, mask_id=0)])
        self.w, self.g, self.weighted = emb.weight, grad, weighted
        self.out = torch.empty(B, D, device="cuda")
        self.plan.bind_inputs([bags])
        self.plan.bind_params([self.w], [self.g])
        self.nbytes = lib.rbx_embed_csr_bwd_workspace_size(self.plan.arr, 1, B)
        self.ws = torch.empty(self.nbytes, dtype=torch.uint8, device="cuda")
        self.lookups = bags.nnz
        self.weights = torch.rand(bags.nnz, device="cuda") * 2 - 1
        self.dw = torch.empty(bags.nnz, device="cuda")
        self.warr, self.dwarr = ops._ptr_array([self.weights]), ops._ptr_array([self.dw])
        self.threshold = ops.bag_long_threshold()
        self.lws, self.lbytes = long_workspace(self.plan, self.threshold)

    def fwd(self):
        T, ws, nb = self.threshold, self.lws.data_ptr(), self.lbytes
        if self.weighted and T > 0:
            _lib.check(lib.rbx_embed_csr_fwd_weighted_long(self.plan.arr, 1, B, T, self.warr, self.out.data_ptr(), D, ws, nb, None,
                                                           ops._stream()))
        elif self.weighted:
            _lib.check(lib.rbx_embed_csr_fwd_weighted(self.plan.arr, 1, B, self.warr, self.out.data_ptr(), D, None, ops._stream()))
        elif T > 0:
            _lib.check(lib.rbx_embed_csr_fwd_long(self.plan.arr, 1, B, T, self.out.data_ptr(), D, None, ws, nb, None, ops._stream()))
        else:
            _lib.check(lib.rbx_embed_csr_fwd(self.plan.arr, 1, B, self.out.data_ptr(), D, None, None, ops._stream()))

    def sort(self):
        if self.weighted:
            _lib.check(lib.rbx_embed_csr_sort_weighted(self.plan.arr, 1, B, self.ws.data_ptr(), self.nbytes, None, ops._stream()))
        else:
            _lib.check(lib.rbx_embed_csr_sort(self.plan.arr, 1, B, self.ws.data_ptr(), self.nbytes, None, ops._stream()))

    def bwd(self):
        if self.weighted:
            _lib.check(lib.rbx_embed_csr_bwd_weighted(self.plan.arr, 1, B, self.warr, self.out.data_ptr(), D, 1, self.ws.data_ptr(),
                                                      self.nbytes, ops._stream()))
        else:
            _lib.check(lib.rbx_embed_csr_bwd(self.plan.arr, 1, B, self.out.data_ptr(), D, None, 1, self.ws.data_ptr(), self.nbytes,
                                             ops._stream()))

    def wgrad(self):
        if self.threshold > 0:
            _lib.check(lib.rbx_embed_csr_weight_grad_long(self.plan.arr, 1, B, self.threshold, self.out.data_ptr(), D, self.dwarr,
                                                          self.lws.data_ptr(), self.lbytes, None, ops._stream()))
        else:
            _lib.check(lib.rbx_embed_csr_weight_grad(self.plan.arr, 1, B, self.out.data_ptr(), D, self.dwarr, None, ops._stream()))


class MaxPool(object):
    """Case 2's bags under POOL_MAX: the forward also stores argpos, the backward reads it beside dY."""

    def __init__(self, emb, grad, bags):
        self.plan = ops.BagPlan([ops.BagSpec("h", D, 0, 0, _lib.POOL_MAX, emb.num_embeddings, mask_id=0)])
        self.w, self.g = emb.weight, grad
        self.out = torch.empty(B, D, device="cuda")
        self.argpos = torch.empty(B, D, dtype=torch.int32, device="cuda")
        self.plan.bind_inputs([bags])
        self.plan.bind_params([self.w], [self.g])
        self.nbytes = lib.rbx_embed_csr_bwd_workspace_size(self.plan.arr, 1, B)
        self.ws = torch.empty(self.nbytes, dtype=torch.uint8, device="cuda")
        self.lookups = bags.nnz
        self.threshold = ops.bag_long_threshold()
        self.lbytes = lib.rbx_embed_csr_fwd_max_workspace_size(self.plan.arr, 1, B, self.threshold)
        self.lws = torch.empty(max(self.lbytes, 1), dtype=torch.uint8, device="cuda")

    def fwd(self):
        _lib.check(lib.rbx_embed_csr_fwd_max(self.plan.arr, 1, B, self.threshold, self.out.data_ptr(), D, self.argpos.data_ptr(), D,
                                             self.lws.data_ptr(), self.lbytes, None, ops._stream()))

    def sort(self):
        _lib.check(lib.rbx_embed_csr_sort_weighted(self.plan.arr, 1, B, self.ws.data_ptr(), self.nbytes, None, ops._stream()))

    def bwd(self):
        _lib.check(lib.rbx_embed_csr_bwd_max(self.plan.arr, 1, B, self.out.data_ptr(), D, self.argpos.data_ptr(), D, 1,
                                             self.ws.data_ptr(), self.nbytes, ops._stream()))


def aten_max(emb, bags, repeats, lines):
    """The routes to a max over the same ids a caller has without this library: forward only, and torch's own
    ``F.embedding_bag(mode="max")`` with its autograd backward (a fresh dense gradient per call)."""
    w, idx, off = emb.weight, bags.indices, bags.offsets
    pad = padded_of(bags)
    lengths = (off[1:] - off[:-1])
    live = (torch.arange(L, device="cuda")[None, :] < lengths[:, None])[:, :, None]
    neg = torch.finfo(torch.float32).min

    def gather_segment():
        with torch.no_grad():
            return torch.segment_reduce(w[idx], "max", offsets=off, axis=0)

    def gather_padded():
        with torch.no_grad():
            return torch.where(live, w[pad], neg).max(dim=1).values

    def bag_fwd():
        with torch.no_grad():
            return torch.nn.functional.embedding_bag(idx, w, off, mode="max", include_last_offset=True)

    dy = torch.rand(B, D, device="cuda")

    def bag_fwd_bwd():
        out = torch.nn.functional.embedding_bag(idx, w, off, mode="max", include_last_offset=True)
        return torch.autograd.grad(out, w, dy)

    names = ["gather + segment_reduce(max)", "padded gather + max(dim=1)", "F.embedding_bag(max) forward",
             "F.embedding_bag(max) forward + autograd backward"]
    res = bracket([gather_segment, gather_padded, bag_fwd, bag_fwd_bwd], repeats)
    lines.append("\nATen over the same ids:\n")
    lines.append("| route | us (min .. max) |")
    lines.append("|---|---|")
    for n, r in zip(names, res):
        lines.append("| %s | %.1f (%.1f .. %.1f) |" % ((n,) + r))
    return res


def bags_of(lengths, rows, gen):
    offsets = torch.zeros(B + 1, dtype=torch.int64)
    torch.cumsum(lengths, 0, out=offsets[1:])
    return ops.Bags(torch.randint(1, rows, (int(offsets[-1]),), generator=gen).cuda(), offsets.cuda())


def padded_of(bags):
    lengths = (bags.offsets[1:] - bags.offsets[:-1])
    ids = torch.zeros(B, L, dtype=torch.int64, device="cuda")
    ids[torch.arange(L, device="cuda")[None, :] < lengths[:, None]] = bags.indices
    return ids


def case(title, names, variants, repeats, lines):
    lines.append("\n### %s\n" % title)
    lines.append("| variant | lookups | forward us (min .. max) | sort us | backward us | sort + backward us |")
    lines.append("|---|---|---|---|---|---|")
    res = [bracket([getattr(v, what) for v in variants], repeats) for what in ("fwd", "sort", "bwd")]
    for k, (n, v) in enumerate(zip(names, variants)):
        f, s, b = res[0][k], res[1][k], res[2][k]
        lines.append("| %s | %d | %.1f (%.1f .. %.1f) | %.1f (%.1f .. %.1f) | %.1f (%.1f .. %.1f) | %.1f |"
                     % (n, v.lookups, f[0], f[1], f[2], s[0], s[1], s[2], b[0], b[1], b[2], s[0] + b[0]))
    if len(variants) == 2:
        lines.append("\nratio %s / %s: forward %.3f, sort %.3f, backward %.3f, sort + backward %.3f"
                     % (names[1], names[0], res[0][1][0] / res[0][0][0], res[1][1][0] / res[1][0][0],
                        res[2][1][0] / res[2][0][0], (res[1][1][0] + res[2][1][0]) / (res[1][0][0] + res[2][0][0])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--rows", type=int, default=10000000)
    ap.add_argument("--out", default="", help="also write the markdown report to this file")
    ap.add_argument("--cases", default="1,2,3,4,5", help="comma-separated case numbers to run")
    ap.add_argument("--threshold", type=int, default=None, help="ops.bag_long_threshold for the run (default: the one in force)")
    a = ap.parse_args()
    if a.threshold is not None:
        ops.bag_long_threshold(a.threshold)
    gen = torch.Generator().manual_seed(7)
    emb = torch.nn.Embedding(a.rows, D).cuda()
    grad = torch.zeros_like(emb.weight)
    try:
        commit = subprocess.run(["git", "rev-parse", "--short", "HEAD"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL,
                                text=True).stdout.strip() or "working tree"
    except OSError:
        commit = "working tree"
    lines = ["box: %s, torch %s; commit: %s; B = %d, table %d x %d, MEAN_ID, %d repeats, variants alternating; long-bag threshold %d"
             % (torch.cuda.get_device_name(0), torch.__version__, commit, B, a.rows, D, a.repeats, ops.bag_long_threshold())]
    want = set(int(c) for c in a.cases.split(","))
    full = bags_of(torch.full((B,), L, dtype=torch.int64), a.rows, gen)
    uni = bags_of(torch.randint(1, L + 1, (B,), generator=gen), a.rows, gen)
    if 1 in want:
        pad = Padded(emb, grad, full.indices.view(B, L))
        case("1. every bag %d ids (the padded call's lookups; `padded again` = its run-to-run spread)" % L,
             ["padded", "CSR", "padded again"], [pad, Ragged(emb, grad, full), Padded(emb, grad, full.indices.view(B, L))],
             a.repeats, lines)
    if 2 in want:
        case("2. lengths uniform in 1 .. %d against the same ids padded to %d" % (L, L), ["padded", "CSR"],
             [Padded(emb, grad, padded_of(uni)), Ragged(emb, grad, uni)], a.repeats, lines)
    if 3 in want:
        skew = torch.randint(1, 10, (B,), generator=gen)
        where = torch.randperm(B, generator=gen)[:B // 1000]
        skew[where] = torch.randint(1000, 5001, (where.numel(),), generator=gen)
        total = int(skew.sum())
        even = torch.full((B,), total // B, dtype=torch.int64)
        even[:total - int(even.sum())] += 1
        skewed = bags_of(skew, a.rows, gen)
        walked, handed = Ragged(emb, grad, skewed, threshold=0), Ragged(emb, grad, skewed)
        case("3. skewed lengths (1 .. 9, 0.1 pct of the bags 1 000 .. 5 000) against the same nnz spread evenly",
             ["even", "skewed, threshold 0", "skewed, threshold %d" % handed.threshold],
             [Ragged(emb, grad, bags_of(even, a.rows, gen)), walked, handed], a.repeats, lines)
        torch.cuda.synchronize()
        short = (skew < max(handed.threshold, 1)).cuda()
        same = torch.equal(walked.out[short], handed.out[short])
        err = float((walked.out - handed.out).abs().max())
        lines.append("\nlong form on the skewed batch: %d bags in %d segments; bags below the threshold bit-equal to threshold 0: "
                     "%s; max |difference| over all bags %.3g" % (long_counts(handed.lws) + (same, err)))
    if 4 in want:
        plain, scored = Weighted(emb, grad, uni, False), Weighted(emb, grad, uni, True)
        case("4. case 2's bags under SUM_ID, unweighted against random per-sample weights", ["unweighted", "weighted"],
             [plain, scored], a.repeats, lines)
        g = bracket([scored.wgrad], a.repeats)[0]
        lines.append("\nweight gradient (memset of dw + bag_walk_kernel<WeightGradOp>): %.1f us (%.1f .. %.1f)" % g)
    if 5 in want:
        case("5. case 2's bags under SUM_ID against POOL_MAX (forward + argpos; position-valued sort; masked reduce)",
             ["sum", "max"], [Weighted(emb, grad, uni, False), MaxPool(emb, grad, uni)], a.repeats, lines)
        aten_max(emb, uni, a.repeats, lines)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
