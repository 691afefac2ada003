"""FiGNN's message-passing step: forward + backward of one layer through (f) the fused op (ops.fignn_step:
csrc/rbx_fignn.hip), (c) the project's composition (ops.fignn_step_torch) and (r) the reference's literal form (gathered
concat through W_attn, broadcast matmul, bmm, nn.GRUCell), and the whole FiGNNInteraction.fignn_layer at n_layers = 3 with
the step kernels on and off.

    python profiles/fignn.py --out profiles/fignn/table.md     # on the GPU; --quick: B = 4096 only

Every form runs in ONE process, interleaved round by round on the same random data; a cell is the median of the rounds with
(min - max) as its run-to-run spread, and the peak memory above what is allocated before the step.  The gates
ops.config.fignn_fields / fignn_dim are raised to the kernels' whole range for the run."""
import argparse
import os
import sys
from itertools import product

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

SHAPES = ((26, 16), (39, 16), (48, 16), (26, 32), (39, 32))


def _literal(h, h0, w_attn, W_out, W_in, bias_p, cell, nodes):
    """fignn.py:119-137 and GraphLayer.forward as the reference writes them."""
    B, F, A = h.shape
    src, dst = nodes
    concat = torch.cat([h0[:, src, :], h0[:, dst, :]], dim=-1)
    alpha = torch.nn.functional.leaky_relu(concat @ w_attn.view(2 * A, 1), 0.01).view(B, F, F)
    alpha = alpha.masked_fill(torch.eye(F, dtype=torch.bool, device=h.device), float("-inf"))
    g = torch.softmax(alpha, dim=-1)
    h_out = torch.matmul(W_out, h.unsqueeze(-1)).squeeze(-1)
    a = torch.matmul(W_in, torch.bmm(g, h_out).unsqueeze(-1)).squeeze(-1) + bias_p
    return cell(a.view(-1, A), h.reshape(-1, A)).view(B, F, A) + h0


def _round_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def _measure(forms, iters, rounds):
    """{name: (median ms, min ms, max ms, peak MiB) or None when out of memory}: the forms interleaved round by round."""
    out, alive = {}, {}
    for name, fn in forms.items():
        try:
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            fn()
            fn()
            torch.cuda.synchronize()
            alive[name] = ((torch.cuda.max_memory_allocated() - base) / 2.0 ** 20, [])
        except torch.cuda.OutOfMemoryError:
            torch.cuda.empty_cache()
            out[name] = None
    for _ in range(rounds):
        for name in alive:
            alive[name][1].append(_round_ms(forms[name], iters))
    for name, (peak, t) in alive.items():
        t.sort()
        out[name] = (t[len(t) // 2], t[0], t[-1], peak)
    return out


def step_rows(quick):
    from recbox_amd import ops
    rows = []
    for B in ((4096,) if quick else (4096, 65536)):
        for F, A in SHAPES:
            torch.manual_seed(B + F + A)
            dev = "cuda"
            h0 = torch.relu(torch.randn(B, F, A, device=dev)).requires_grad_()
            h = torch.randn(B, F, A, device=dev).requires_grad_()
            up = torch.randn(B, F, A, device=dev)
            cell = torch.nn.GRUCell(A, A).to(dev)
            w_attn = (torch.randn(2 * A, device=dev) / (2 * A) ** 0.5).requires_grad_()
            W_out = (torch.randn(F, A, A, device=dev) / A ** 0.5).requires_grad_()
            W_in = (torch.randn(F, A, A, device=dev) / A ** 0.5).requires_grad_()
            bias_p = torch.zeros(A, device=dev).requires_grad_()
            ws = (w_attn, W_out, W_in, bias_p, cell.weight_ih, cell.weight_hh, cell.bias_ih, cell.bias_hh)
            src, dst = (list(t) for t in zip(*product(range(F), repeat=2)))
            leaves = (h, h0) + ws

            def step(form):
                if form == "f":
                    y = ops.fignn_step(h, h0, *ws)[0]
                elif form == "c":
                    y = ops.fignn_step_torch(h, h0, *ws)[0]
                else:
                    y = _literal(h, h0, w_attn, W_out, W_in, bias_p, cell, (src, dst))
                torch.autograd.grad((y * up).sum(), leaves)

            forms = {"f": lambda: step("f"), "c": lambda: step("c")}
            if ops.fignn_step_supported(F, A) is False:
                forms.pop("f")
            forms["r"] = lambda: step("r")
            iters, rounds = (10, 7) if B == 4096 else (3, 5)
            rows.append((B, F, A, _measure(forms, iters, rounds)))
            print(rows[-1], flush=True)
            del h, h0, up, cell, ws, leaves
            torch.cuda.empty_cache()
    return rows


def layer_rows(quick):
    from recbox_amd import ops
    from recbox_amd.recbole import FiGNNInteraction
    out = []
    for B in ((4096,) if quick else (4096, 65536)):
        for F, A in ((26, 16), (39, 16)):
            torch.manual_seed(0)
            m = FiGNNInteraction(F, 16, A, 3, 2, 0.0, 0.0).cuda().train()
            x = torch.randn(B, F, 16, device="cuda").requires_grad_()

            def step(on):
                ops.config.fignn_fused = on
                torch.autograd.grad(m.fignn_layer(x).sum(), [x] + list(m.parameters()))
                ops.config.fignn_fused = True

            out.append((B, F, A, _measure({"fused": lambda: step(True), "composition": lambda: step(False)}, 5, 5)))
            print(out[-1], flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from recbox_amd import ops
    ops.config.fignn_fields, ops.config.fignn_dim = ops.FIGNN_MAX_FIELDS, ops.FIGNN_MAX_DIM
    fmt = lambda r: "out of memory" if r is None else "%.3f (%.3f - %.3f) ms / %.0f MiB" % r   # noqa: E731
    ratio = lambda r, f: "n/a" if r is None or f is None else "%.2fx" % (r[0] / f[0])          # noqa: E731
    lines = ["| B | F | A | fused fwd+bwd / peak | (c) fignn_step_torch | (r) reference's literal form | vs (c) | vs (r) |",
             "|---|---|---|---|---|---|---|---|"]
    for B, F, A, res in step_rows(a.quick):
        f, c, r = res.get("f"), res.get("c"), res.get("r")
        lines.append("| %d | %d | %d | %s | %s | %s | %s | %s |" % (B, F, A, fmt(f), fmt(c), fmt(r), ratio(c, f), ratio(r, f)))
    lines += ["", "FiGNNInteraction.fignn_layer forward + backward (D = 16, 3 layers = 2 steps, 2 heads, no dropout), the step kernels "
              "on and off (the first stage is ops.field_attn under its own default gates in both):", "",
              "| B | F | A | steps fused | steps composed | ratio |", "|---|---|---|---|---|---|"]
    for B, F, A, res in layer_rows(a.quick):
        lines.append("| %d | %d | %d | %s | %s | %s |" % (B, F, A, fmt(res["fused"]), fmt(res["composition"]),
                                                       ratio(res["composition"], res["fused"])))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
