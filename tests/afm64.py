"""float64 restatement of AFM's pair-attention pooling (helper of tests/test_afm_host.py and tests/test_gpu_afm.py, not a test).

    p_k = x_i * x_j over the P = F (F - 1) / 2 pairs k = (i, j), i < j, row-major      pre_k = W p_k
    s_k = sum_a h_a relu(pre_k)_a      a = softmax_k(s)      out = sum_k a_k p_k

``reference`` states the forward and the backward by hand (no autograd) in float64 or, with ``dtype=torch.float32``, the same
lines in fp32 on the CPU -- the ``ref32`` of tests/fp32_bar.py.  The loss every test uses is ``sum(out * up)``; ``run``
evaluates it through the op under test.

``make_case`` draws ``x`` and ``W`` on the dyadic grid: multiples of 1/8 in [-2, 2].  Every product x_i x_j W is then a
multiple of 1/512 and every pre-activation, a sum of at most 64 of them, a multiple of 1/512 below 2^15: exact in fp32 in ANY
summation order, exact zeros included.  No ReLU unit can flip between two orders (a flipped unit changes dW discontinuously,
and no tolerance covers that), and the exact zeros check the strict ``pre > 0`` of the backward: with more than two fields every fourth
sample's last field is all zero, so its pairs have pre-activations of exactly 0 (a ``>=`` there would put ``ds h W`` into the
other side's dx).  ``make_case`` asserts the exactness on the CPU and counts the zeros.  ``h`` and the upstream gradient are Gaussians; ``h`` is scaled by ``h_scale`` (default 0.1: the logits
then have a spread of a few units, so the softmax is neither uniform nor one-hot; 4.0 gives logits of magnitude about 90)."""
import itertools

import torch


def pairs(F):
    return list(itertools.combinations(range(F), 2))


def _grid(shape, g):
    return torch.randint(-16, 17, shape, generator=g).float() / 8.0


def make_case(B, F, D, A, seed=0, h_scale=0.1, up_scale=1.0, nonpos=False):
    """Inputs of one case, fp32 on the CPU.  ``nonpos``: x >= 0 and W = -|W|, so that every pre-activation is <= 0."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * F + D + A)
    x, w = _grid((B, F, D), g), _grid((A, D), g)
    if nonpos:
        x, w = x.abs(), -w.abs()
    if F > 2:
        x[::4, F - 1] = 0                      # pairs with an all-zero side: pre-activations that are exactly 0 (dx shows a >= 0)
    case = {"x": x, "w": w, "h": torch.randn(A, generator=g) * h_scale, "up": torch.randn(B, D, generator=g) * up_scale,
            "dims": (B, F, D, A)}
    pp = pairs(F)
    I, J = torch.tensor([i for i, _ in pp]), torch.tensor([j for _, j in pp])
    pre32 = (x[:, I] * x[:, J]) @ w.t()
    pre64 = (x.double()[:, I] * x.double()[:, J]) @ w.double().t()
    assert torch.equal(pre32.double(), pre64), "pre-activations are not exact in fp32"
    case["zeros"] = int((pre64 == 0).sum())
    return case


def reference(case, dtype=torch.float64):
    """{"out", "attn", "dx", "dW", "dh"} of ``sum(out * up)``, by hand, in ``dtype`` on the CPU."""
    B, F, D, A = case["dims"]
    x, w, h, up = (case[k].detach().cpu().to(dtype) for k in ("x", "w", "h", "up"))
    pp = pairs(F)
    I, J = torch.tensor([i for i, _ in pp]), torch.tensor([j for _, j in pp])
    xi, xj = x[:, I], x[:, J]
    p = xi * xj                                                                 # [B, P, D]
    pre = p @ w.t()                                                             # [B, P, A]
    r = torch.relu(pre)
    s = r @ h                                                                   # [B, P]
    a = torch.softmax(s, dim=1)
    out = (a.unsqueeze(2) * p).sum(1)

    gk = (p * up.unsqueeze(1)).sum(2)                                           # dout . p_k
    G = (up * out).sum(1, keepdim=True)
    ds = a * (gk - G)
    dpre = ds.unsqueeze(2) * h * (pre > 0).to(dtype)
    dp = a.unsqueeze(2) * up.unsqueeze(1) + dpre @ w
    dx = torch.zeros_like(x)
    dx.index_add_(1, I, dp * xj)
    dx.index_add_(1, J, dp * xi)
    dW = torch.einsum("bpa,bpd->ad", dpre, p)
    dh = (ds.unsqueeze(2) * r).sum((0, 1))
    return {"out": out, "attn": a, "dx": dx, "dW": dW, "dh": dh}


NAMES = ("out", "attn", "dx", "dW", "dh")


def run(fn, case, device, x=None, up=None, want_attn=True, needs=(True, True, True)):
    """The same loss through ``fn(x, w, h, want_attn) -> (out, attn)`` on ``device``.  ``x``: a prepared ``(tensor, leaf)`` to
    use instead of the case's x (a strided view); ``up``: a prepared upstream gradient on ``device`` (a non-contiguous one);
    ``needs``: which of (x, w, h) require a gradient.  Returns the dict of ``reference`` (None where nothing was asked)."""
    w = case["w"].detach().clone().to(device).requires_grad_(needs[1])
    h = case["h"].detach().clone().to(device).requires_grad_(needs[2])
    if x is None:
        x = case["x"].detach().clone().to(device).requires_grad_(needs[0])
        xleaf = x
    else:
        x, xleaf = x
    up = case["up"].to(device) if up is None else up
    out, attn = fn(x, w, h, want_attn)
    if any(needs):
        (out * up).sum().backward()
    return {"out": out.detach(), "attn": attn.detach() if attn is not None else None, "dx": xleaf.grad, "dW": w.grad,
            "dh": h.grad}
