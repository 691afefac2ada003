"""Dynamic routing of the multi-interest capsule layer restated in torch (helper of the capsule tests, not a test).  Every
function works in the dtype and on the device of its inputs: float64 on the CPU is the bound the kernels are measured
against, float32 on the GPU is the einsum composition that runs through the same asserts.

Positions l = 0..L-1 of a user's history x [B, L, D] are transformed into K "prediction vectors" each:
  type 0   hat[b, k, l] = A x[b, l]                one Linear(D, D), the same for every interest
  type 1   hat[b, k, l] = A_k x[b, l]              one Linear(D, K D)
  type 2   hat[b, k, l] = W[l, k D:(k + 1) D] x[b, l]     a matrix per position and interest (W [L, K D, D])
Routing, per (b, k) and independent of every other pair: with logits z[l] (zeros, or for type 0 a given random start),
  c = softmax_l(z), set to 0 at padded positions without renormalising;  s = sum_l c[l] hat[l];
  v = squash(s) = |s|^2 / (1 + |s|^2) / sqrt(|s|^2 + 1e-9) s;   z += hat v.
Iterations 0 and 1 update z and see hat as a constant; from iteration 2 on nothing is updated and hat carries the gradient,
so the result of ``routing_times`` >= 3 is iteration 2's v with c a constant, and fewer iterations give a constant."""
import torch


def transform(x, weight, btype, K):
    """hat as [B, K, L, D]."""
    B, L, D = x.shape
    if btype == 2:
        w = weight.reshape(-1, K * D, D)[:L]
        hat = torch.einsum("lnd,bld->bln", w, x)
    else:
        hat = x @ weight.t()
        if btype == 0:
            return hat.unsqueeze(1).expand(B, K, L, D)
    return hat.reshape(B, L, K, D).transpose(1, 2)


def squash(s):
    n = (s * s).sum(-1, keepdim=True)
    return n / (1 + n) / torch.sqrt(n + 1e-9) * s


def route(hat, mask, routing_times=3, init=None):
    """hat [B, K, L, D], mask [B, L] (0 = padding), init [B, K, L] or None -> v [B, K, D]."""
    B, K, L, D = hat.shape
    z = init.to(hat.dtype) if init is not None else torch.zeros(B, K, L, dtype=hat.dtype, device=hat.device)
    keep = (mask.reshape(B, 1, L) != 0).to(hat.dtype)
    const = hat.detach()
    v = None
    for i in range(routing_times):
        c = torch.softmax(z, dim=-1) * keep
        v = squash(torch.einsum("bkl,bkld->bkd", c, const if i < 2 else hat))
        if i < 2:
            z = z + torch.einsum("bkld,bkd->bkl", const, v)
    return v


def capsule_forward(x, mask, weight, btype, K, routing_times=3, init=None):
    return route(transform(x, weight, btype, K), mask, routing_times, init)
