"""float64 restatement of one FiGNN message-passing step and its gradients (helper of tests/test_fignn_host.py and
tests/test_gpu_fignn.py, not a test).  Per sample, h, h0 [F, A]:

    s_i = w_attn[:A] . h0_i     d_j = w_attn[A:] . h0_j     g[i, :] = softmax_j leaky_relu(s_i + d_j, 0.01), g[i, i] = 0
    hout_j = W_out[j] h_j       aggr_i = sum_j g[i, j] hout_j        a_i = W_in[i] aggr_i + bias_p
    r = sig(W_ir a + b_ir + W_hr h + b_hr)   z = sig(W_iz a + b_iz + W_hz h + b_hz)   n = tanh(W_in a + b_in + r (W_hn h + b_hn))
    h'_i = (1 - z) n + z h_i + h0_i

``forward`` states this in the reference's literal form -- the gathered source / destination rows, their concat through
``w_attn``, the broadcast matrix-vector products, the gates written out -- in a chosen dtype on the CPU, so it shares no code
with ``ops.fignn_step_torch``.  ``reference`` is that in float64 with its gradients of ``sum(y * up)``; ``ref32`` the same in
float32 (the ``ref32`` of tests/fp32_bar.py); ``run`` evaluates the loss through the op under test.

``make_case`` draws Gaussians: h, h0 and up standard (``same``: h IS h0, as in the first layer), w_attn with deviation
1 / sqrt(2 A) times ``w_scale``, the matrices with 1 / sqrt(A), the biases times 0.5.  It refuses a seed when a leaky-relu
argument of the float64 forward lies within 1e-4 of zero, so that fp32 rounding cannot flip a slope."""
import math
from itertools import product

import torch

WEIGHTS = ("w_attn", "W_out", "W_in", "bias_p", "w_ih", "w_hh", "b_ih", "b_hh")
GRADS = ("dh", "dh0") + tuple("d" + n for n in WEIGHTS)
NAMES = ("y", "g") + GRADS
MIN_PRE_LEAKY = 1e-4


def forward(h, h0, w_attn, W_out, W_in, bias_p, w_ih, w_hh, b_ih, b_hh):
    """(y, g, the leaky-relu arguments [B, F, F]) in the dtype of the tensors, fignn.py:119-137 line by line."""
    B, F, A = h.shape
    src, dst = zip(*list(product(range(F), repeat=2)))
    concat = torch.cat([h0[:, list(src), :], h0[:, list(dst), :]], dim=-1)                   # [B, F F, 2 A]
    pre = (concat @ w_attn.reshape(2 * A, 1)).view(B, F, F)
    alpha = torch.where(pre > 0, pre, 0.01 * pre)
    alpha = alpha.masked_fill(torch.eye(F, dtype=torch.bool), float("-inf"))
    g = torch.softmax(alpha, dim=-1)
    hout = torch.matmul(W_out, h.unsqueeze(-1)).squeeze(-1)
    a = torch.matmul(W_in, torch.bmm(g, hout).unsqueeze(-1)).squeeze(-1) + bias_p
    a2, h2 = a.reshape(-1, A), h.reshape(-1, A)
    gi, gh = a2 @ w_ih.t() + b_ih, h2 @ w_hh.t() + b_hh
    r = 1.0 / (1.0 + torch.exp(-(gi[:, :A] + gh[:, :A])))
    z = 1.0 / (1.0 + torch.exp(-(gi[:, A:2 * A] + gh[:, A:2 * A])))
    n = torch.tanh(gi[:, 2 * A:] + r * gh[:, 2 * A:])
    y = ((1.0 - z) * n + z * h2).view(B, F, A) + h0
    return y, g, pre


def _off_diagonal_min(pre):
    F = pre.shape[1]
    return float(pre.abs().masked_fill(torch.eye(F, dtype=torch.bool), float("inf")).min())


def make_case(B, F, A, seed=0, same=False, w_scale=1.0, up_scale=1.0):
    for s in range(seed, seed + 400):
        g = torch.Generator().manual_seed(100003 * s + 1009 * B + 31 * F + 7 * A + int(same))
        case = {"dims": (B, F, A), "same": same,
                "h0": torch.randn(B, F, A, generator=g),
                "w_attn": torch.randn(2 * A, generator=g) * (w_scale / math.sqrt(2 * A)),
                "W_out": torch.randn(F, A, A, generator=g) / math.sqrt(A),
                "W_in": torch.randn(F, A, A, generator=g) / math.sqrt(A),
                "bias_p": torch.randn(A, generator=g) * 0.5,
                "w_ih": torch.randn(3 * A, A, generator=g) / math.sqrt(A),
                "w_hh": torch.randn(3 * A, A, generator=g) / math.sqrt(A),
                "b_ih": torch.randn(3 * A, generator=g) * 0.5,
                "b_hh": torch.randn(3 * A, generator=g) * 0.5,
                "up": torch.randn(B, F, A, generator=g) * up_scale}
        case["h"] = case["h0"] if same else torch.randn(B, F, A, generator=g)
        pre = forward(*(case[n].double() for n in ("h", "h0") + WEIGHTS))[2]
        if _off_diagonal_min(pre) > MIN_PRE_LEAKY:
            return case
    raise RuntimeError("no seed keeps every leaky-relu argument away from zero for %s" % ((B, F, A),))


def run(fn, case, device, want_graph=True, needs=None, dtype=None):
    """The loss ``sum(y * up)`` through ``fn(h, h0, *weights, want_graph) -> (y, g)`` on ``device``.  ``needs``: which of
    (h, h0) + WEIGHTS require a gradient (default all).  With ``case["same"]`` one leaf serves as h and h0: ``dh`` is then the
    sum of both gradients and ``dh0`` None.  Returns {"y", "g", "dh", "dh0", "dw_attn", ...}."""
    needs = (True,) * 10 if needs is None else needs
    names = ("h", "h0") + WEIGHTS

    def leaf(n, need):
        t = case[n].detach().clone().to(device)
        return (t.to(dtype) if dtype is not None else t).requires_grad_(need)
    t = {n: leaf(n, needs[i]) for i, n in enumerate(names)}
    if case["same"]:
        t["h0"] = t["h"]
    up = case["up"].to(device)
    up = up.to(dtype) if dtype is not None else up
    y, g = fn(*[t[n] for n in names], want_graph)
    if any(needs):
        (y * up).sum().backward()
    out = {"y": y.detach(), "g": g.detach() if g is not None else None}
    for n in names:
        out["d" + n] = t[n].grad
    if case["same"]:
        out["dh0"] = None
    return out


def _literal(*a):
    y, g, _ = forward(*a[:10])
    return y, (g if a[10] else None)


def reference(case):
    """The dict of ``run`` in float64 on the CPU through ``forward``."""
    return run(_literal, case, "cpu", dtype=torch.float64)


def ref32(case):
    """The same in float32 with plain torch ops on the CPU."""
    return run(_literal, case, "cpu", dtype=torch.float32)
