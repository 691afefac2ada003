"""Float64 restatement of the self-attentive multi-interest pooling (third_party/rechub/basic/layers.py:541-550), on the CPU:

    Hid = tanh(x W1)   S = Hid W2 masked   A = softmax over L of S   out = A^T x

The reference adds ``-1e9 (1 - mask)`` to the logits in fp32.  For |logit| < 32 that sum IS -1e9 at a masked position (the
spacing of floats at 1e9 is 64) while autograd passes the gradient through the addition unchanged.  Float64 would keep the
logit beside the -1e9, so the masked logits are restated as ``a + (1 - m) (-1e9 - a.detach())``: exactly -1e9 in the forward,
identity gradient in the backward -- the fp32 behaviour for |a| < 32, which every case drawn here satisfies.  A fully masked
sample therefore attends uniformly (A = 1 / L) and still carries gradient; positions masked in a partly masked sample get
A = 0 and no gradient on their own.

Measured with the draws of ``make_case`` (x ~ N(0, 1), W1 ~ N(0, 1) / sqrt(D), W2 ~ N(0, 1) / sqrt(H), lengths uniform in
0..L, upstream gradients ~ N(0, 1) / sqrt(B)) over the shapes of tests/test_gpu_sa.py at B = 301, the fp32 ATen composition
(``ops.sa_pool_torch``) is within 7e-7 (out), 6e-8 (dx), 4e-7 (dW1) and 1.4e-6 (dW2) of this restatement; with unscaled
gradients dW2 reaches 2.8e-5, hence the 1 / sqrt(B)."""
import torch


def sa_forward(x, w1, w2, mask=None, pool=True):
    """(out [B, K, D] or None, attn [B, L, K]) in the dtype of ``x`` (float64 here)."""
    B, L, _ = x.shape
    a = torch.tanh(x @ w1) @ w2
    if mask is not None:
        m = mask.reshape(B, L, 1).to(x.dtype)
        a = a + (1 - m) * (-1.0e9 - a.detach())
    attn = torch.softmax(a, dim=1)
    return (attn.transpose(1, 2) @ x if pool else None), attn


def make_case(B, L, D, H, K, seed=0):
    """fp32 CPU tensors: x, w1, w2, a long mask from lengths uniform in 0..L (sample 0 empty and sample 1 full when there are
    that many), and the upstream gradients g_out [B, K, D], g_attn [B, L, K]."""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * L + 31 * D + H + K + B)
    x = torch.randn(B, L, D, generator=g)
    w1 = torch.randn(D, H, generator=g) / D ** 0.5
    w2 = torch.randn(H, K, generator=g) / H ** 0.5
    lengths = torch.randint(0, L + 1, (B,), generator=g)
    lengths[0] = 0
    if B > 1:
        lengths[1] = L
    mask = (torch.arange(L).unsqueeze(0) < lengths.unsqueeze(1)).long()
    g_out = torch.randn(B, K, D, generator=g) / B ** 0.5
    g_attn = torch.randn(B, L, K, generator=g) / B ** 0.5
    return {"x": x, "w1": w1, "w2": w2, "mask": mask, "g_out": g_out, "g_attn": g_attn}


def reference(case, use_out=True, use_attn=True, masked=True):
    """The float64 results for a case of ``make_case``: out, attn, dx, dw1, dw2 with the chosen upstream gradients."""
    x, w1, w2 = (case[n].double().requires_grad_(True) for n in ("x", "w1", "w2"))
    out, attn = sa_forward(x, w1, w2, case["mask"] if masked else None)
    loss = 0.0
    if use_out:
        loss = loss + (out * case["g_out"].double()).sum()
    if use_attn:
        loss = loss + (attn * case["g_attn"].double()).sum()
    dx, dw1, dw2 = torch.autograd.grad(loss, (x, w1, w2))
    return {"out": out.detach(), "attn": attn.detach(), "dx": dx, "dw1": dw1, "dw2": dw2}


def run(fn, case, device="cpu", use_out=True, use_attn=True, masked=True, mask=None):
    """The same five results from ``fn(x, w1, w2, mask) -> (out, attn)`` in fp32 on ``device``."""
    x, w1, w2 = (case[n].to(device).requires_grad_(True) for n in ("x", "w1", "w2"))
    if mask is None:
        mask = case["mask"].to(device) if masked else None
    out, attn = fn(x, w1, w2, mask)
    loss = 0.0
    if use_out:
        loss = loss + (out * case["g_out"].to(device)).sum()
    if use_attn:
        loss = loss + (attn * case["g_attn"].to(device)).sum()
    dx, dw1, dw2 = torch.autograd.grad(loss, (x, w1, w2))
    return {"out": out.detach(), "attn": attn.detach(), "dx": dx, "dw1": dw1, "dw2": dw2}
