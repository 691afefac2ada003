"""Float64 restatement of the additive attention pooling of the session-based models (third_party/rechub/models/matching/
narm.py:60-68, stamp.py:69-72), on the CPU:

    q = sigmoid(x W^T + ctx) v     e = exp(q) mask (as written: no max subtraction)     alpha = e / max(sum_l e, eps)
    out = sum_l alpha x

and of STAMP's scores (stamp.py:55-83) over a state_dict.  ``alpha`` carries no gradient of its own (the op returns it
non-differentiable); the gradients are those of ``out``.

Measured with the draws of ``make_case`` (x ~ N(0, 1), W ~ N(0, 1) / sqrt(D), v ~ N(0, 1) / sqrt(H), ctx ~ N(0, 1), lengths
uniform in 1..L, upstream gradient ~ N(0, 1) / sqrt(B)) at every (L, D, H) of tests/test_gpu_addattn.py and B = 1 and 37, the
fp32 ATen composition (``ops.additive_attn_pool_torch``, CPU) is within 2.1e-7 (out), 5.7e-8 (alpha), 2.6e-8 (dx), 1.7e-7 (dW),
1.5e-8 (dctx) and 7.4e-7 (dv) of this restatement, with eps = 0 and eps = 1e-12 alike.  The tests use the project's absolute
1e-4; the composition sits far within a tenth of it, so the draws needed no rescaling."""
import torch


def forward(x, w, ctx, v, mask=None, eps=0.0):
    """(out [B, D], alpha [B, L]) in the dtype of ``x`` (float64 here)."""
    B, L, _ = x.shape
    pre = x @ w.t()
    if ctx is not None:
        pre = pre + ctx.unsqueeze(1)
    e = torch.exp(torch.sigmoid(pre) @ v.reshape(-1))
    if mask is not None:
        e = e * (mask.reshape(B, L) != 0).to(x.dtype)
    total = e.sum(dim=1, keepdim=True)
    alpha = e / (total.clamp_min(eps) if eps > 0 else total)
    return (alpha.unsqueeze(-1) * x).sum(1), alpha


def make_case(B, L, D, H, seed=0):
    """fp32 CPU tensors: x, w, ctx, v, a long mask from lengths uniform in 1..L (sample 0 of length 1 and sample 1 of length L
    when there are that many) and the upstream gradient g_out [B, D]."""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * L + 31 * D + H + B)
    x = torch.randn(B, L, D, generator=g)
    w = torch.randn(H, D, generator=g) / D ** 0.5
    v = torch.randn(H, generator=g) / H ** 0.5
    assert v.abs().sum().item() <= 16.0                      # exp(q) as written overflows only beyond |v|_1 = 88
    ctx = torch.randn(B, H, generator=g)
    lengths = torch.randint(1, L + 1, (B,), generator=g)
    lengths[0] = 1
    if B > 1:
        lengths[1] = L
    mask = (torch.arange(L).unsqueeze(0) < lengths.unsqueeze(1)).long()
    g_out = torch.randn(B, D, generator=g) / B ** 0.5
    return {"x": x, "w": w, "ctx": ctx, "v": v, "mask": mask, "g_out": g_out}


NAMES = ("out", "alpha", "dx", "dw", "dctx", "dv")


def reference(case, use_ctx=True, masked=True, eps=0.0):
    """The float64 results for a case of ``make_case``: out, alpha, dx, dw, dctx (None without ctx), dv."""
    x, w, c, v = (case[n].double().requires_grad_(True) for n in ("x", "w", "ctx", "v"))
    out, alpha = forward(x, w, c if use_ctx else None, v, case["mask"] if masked else None, eps)
    leaves = (x, w, c, v) if use_ctx else (x, w, v)
    grads = list(torch.autograd.grad((out * case["g_out"].double()).sum(), leaves))
    if not use_ctx:
        grads.insert(2, None)
    return dict(zip(NAMES, [out.detach(), alpha.detach()] + grads))


def run(fn, case, device="cpu", use_ctx=True, masked=True, eps=0.0, mask=None, x=None):
    """The same six results from ``fn(x, w, ctx, v, mask, eps) -> (out, alpha)`` in fp32 on ``device``.  ``mask`` / ``x``
    replace the case's (another dtype; a strided view holding the same values, already a leaf on ``device``)."""
    if x is None:
        x = case["x"].to(device).requires_grad_(True)
    w, c, v = (case[n].to(device).requires_grad_(True) for n in ("w", "ctx", "v"))
    if mask is None:
        mask = case["mask"].to(device) if masked else None
    out, alpha = fn(x, w, c if use_ctx else None, v, mask, eps)
    leaves = (x, w, c, v) if use_ctx else (x, w, v)
    grads = list(torch.autograd.grad((out * case["g_out"].to(device)).sum(), leaves))
    if not use_ctx:
        grads.insert(2, None)
    return dict(zip(NAMES, [out.detach(), alpha.detach()] + grads))


def stamp_scores(sd, ids):
    """z [B, V] of stamp.py:55-83 from a state_dict (tensors of any float dtype, possibly requiring grad) and ids [B, L]."""
    table = sd["item_emb.weight"]
    value_mask = (ids != 0).unsqueeze(-1)
    counts = value_mask.sum(dim=1)                                             # [B, 1]
    emb = table[ids] * value_mask
    x_t = table[torch.gather(ids, 1, counts - 1)]                              # [B, 1, D]
    m_s = (emb.sum(1) / counts).unsqueeze(1)
    q = torch.sigmoid(emb @ sd["w_1_t"] + x_t @ sd["w_2_t"] + m_s @ sd["w_3_t"] + sd["b_a"]) @ sd["w_0"]
    e = torch.exp(q) * value_mask
    a = e / e.abs().sum(dim=1, keepdim=True).clamp_min(1e-12)
    m_a = (a * emb).sum(1) + m_s.squeeze(1)
    h_s = torch.tanh(m_a) @ sd["f_s.1.weight"].t() + sd["f_s.1.bias"]
    h_t = (torch.tanh(x_t) @ sd["f_t.1.weight"].t() + sd["f_t.1.bias"]).squeeze(1)
    return (h_s * h_t) @ table.t()
