"""float64 restatement of Caser's convolutional layers and their gradients (helper of tests/test_caser_host.py and
tests/test_gpu_caser.py, not a test).  x [B, L, D], w_v [n_v, 1, L, 1], b_v [n_v], w_h[h - 1] [n_h, 1, h, D], b_h[h - 1] [n_h]:

    out[b, v D + d]                 = b_v[v] + sum_l w_v[v, 0, l, 0] x[b, l, d]
    out[b, n_v D + (h - 1) n_h + f] = max_{t <= L - h} relu(b_h[h - 1][f] + sum_{i < h, d} w_h[h - 1][f, 0, i, d] x[b, t + i, d])

``forward`` states this without a convolution -- the windows of height h are gathered with ``unfold`` and multiplied with the
flattened filters -- in a chosen dtype on the CPU, so it shares no code with ``ops.caser_conv_torch``.  ``reference`` is that in
float64 with its gradients of ``sum(out * up)``; ``ref32`` the same in float32 (the ``ref32`` of tests/fp32_bar.py); ``run``
evaluates the loss through the op under test.

The max over time and the ReLU make the gradient discontinuous, so ``make_case`` draws inputs for which, in float64, every
(b, h, f) has its best window at least ``MARGIN`` = 1e-4 above the runner-up and at least 1e-4 away from zero, both relative to
the largest pre-activation of the case.  x, up and the biases (times 0.5) are Gaussians, w_h[h - 1] has deviation 1 / sqrt(h D)
and w_v 1 / sqrt(L).  A batch of B L n_h triples cannot be clean as a whole at any seed (about one triple in a thousand is not),
so the SAMPLES that hold an offending triple are drawn again, from the same generator, until none is left; the condition is
then asserted over the whole case."""
import math

import torch

MARGIN = 1e-4
MAX_ROUNDS = 400


def names(L, n_h, n_v):
    """The gradient names of a case in the order of ``run``'s leaves."""
    out = ["dx"]
    if n_v:
        out += ["dw_v", "db_v"]
    if n_h:
        out += ["dw_h%d" % i for i in range(L)] + ["db_h%d" % i for i in range(L)]
    return tuple(out)


def forward(x, w_v, b_v, w_h, b_h):
    """(out, pre) in the dtype of the tensors; ``pre[h - 1]`` [B, L - h + 1, n_h] are the pre-activations with their bias."""
    B, L, D = x.shape
    pieces, pre = [], []
    if w_v is not None:
        n_v = w_v.shape[0]
        pieces.append(((w_v.reshape(n_v, L, 1).unsqueeze(0) * x.unsqueeze(1)).sum(2) + b_v.reshape(1, n_v, 1)).reshape(B, n_v * D))
    for i, (w, b) in enumerate(zip(w_h, b_h)):
        h, n_h = i + 1, w.shape[0]
        windows = x.unfold(1, h, 1).permute(0, 1, 3, 2).reshape(B, L - h + 1, h * D)          # [B, t, (i, d)]
        p = windows @ w.reshape(n_h, h * D).t() + b
        pre.append(p)
        pieces.append(torch.where(p > 0, p, torch.zeros_like(p)).max(dim=1).values)
    return torch.cat(pieces, 1), pre


def _offenders(pre):
    """(per-sample flag of a triple within MARGIN of a tie or of zero, the largest |pre-activation|)."""
    top = max(float(p.abs().max()) for p in pre)
    bad = torch.zeros(pre[0].shape[0], dtype=torch.bool)
    for p in pre:
        best = p.topk(min(2, p.shape[1]), dim=1).values                                       # [B, 1 or 2, n_h]
        bad |= (best[:, 0].abs() < MARGIN * top).any(-1)
        if best.shape[1] == 2:
            bad |= (best[:, 0] - best[:, 1] < MARGIN * top).any(-1)
    return bad, top


def make_case(B, L, D, n_h, n_v, seed=0, up_scale=1.0):
    g = torch.Generator().manual_seed(100003 * seed + 1009 * B + 131 * L + 31 * D + 7 * n_h + n_v)
    case = {"dims": (B, L, D, n_h, n_v),
            "w_v": torch.randn(n_v, 1, L, 1, generator=g) / math.sqrt(L) if n_v else None,
            "b_v": torch.randn(n_v, generator=g) * 0.5 if n_v else None,
            "w_h": [torch.randn(n_h, 1, h, D, generator=g) / math.sqrt(h * D) for h in range(1, L + 1)] if n_h else [],
            "b_h": [torch.randn(n_h, generator=g) * 0.5 for _ in range(L)] if n_h else [],
            "up": torch.randn(B, n_v * D + n_h * L, generator=g) * up_scale}
    x = torch.randn(B, L, D, generator=g)
    if n_h:
        w64, b64 = [w.double() for w in case["w_h"]], [b.double() for b in case["b_h"]]
        for _ in range(MAX_ROUNDS):
            bad, _ = _offenders(forward(x.double(), None, None, w64, b64)[1])
            if not bad.any():
                break
            x[bad] = torch.randn(int(bad.sum()), L, D, generator=g)
        bad, top = _offenders(forward(x.double(), None, None, w64, b64)[1])
        assert not bad.any(), "no draw keeps every winner %g clear of the runner-up and of zero for %s" % (MARGIN, case["dims"])
        case["top"] = top
    case["x"] = x
    return case


def run(fn, case, device, dtype=None, x_view=None):
    """The loss ``sum(out * up)`` through ``fn(x, w_v, b_v, w_h, b_h) -> out`` on ``device``.  ``x_view(leaf)`` may return the
    view of a wider leaf that is passed as x; the gradient reported is then ``x_view`` of the leaf's.  Returns {"out", "dx",
    "dw_v", "db_v", "dw_h0", ..., "db_h0", ...}."""
    B, L, D, n_h, n_v = case["dims"]

    def leaf(t):
        t = t.detach().clone().to(device)
        return (t.to(dtype) if dtype is not None else t).requires_grad_()
    w_v, b_v = (leaf(case["w_v"]), leaf(case["b_v"])) if n_v else (None, None)
    w_h, b_h = [leaf(t) for t in case["w_h"]], [leaf(t) for t in case["b_h"]]
    if x_view is None:
        xl = leaf(case["x"])
        x = xl
    else:
        xl, x = x_view(case["x"].to(device), dtype)
    up = case["up"].to(device)
    up = up.to(dtype) if dtype is not None else up
    out = fn(x, w_v, b_v, w_h, b_h)
    (out * up).sum().backward()
    res = {"out": out.detach(), "dx": xl.grad if x_view is None else xl.grad[:, :, :D]}
    if n_v:
        res.update(dw_v=w_v.grad, db_v=b_v.grad)
    for i in range(L if n_h else 0):
        res["dw_h%d" % i], res["db_h%d" % i] = w_h[i].grad, b_h[i].grad
    return res


def _literal(x, w_v, b_v, w_h, b_h):
    return forward(x, w_v, b_v, w_h, b_h)[0]


def reference(case):
    """The dict of ``run`` in float64 on the CPU through ``forward``."""
    return run(_literal, case, "cpu", dtype=torch.float64)


def ref32(case):
    """The same in float32 with plain torch ops on the CPU."""
    return run(_literal, case, "cpu", dtype=torch.float32)
