"""DIN's local activation unit restated with plain torch ops on the CPU (helper of the DIN tests, not a test): the pair-feature
Linear and the masked pooling of csrc/rbx_din.hip, in float64 for the bound and in float32 for the bar of tests/fp32_bar.py,
the case builders the GPU form tests and tests/test_fp32_bar_host.py share, and the two backward passes written out by hand
(the formulas in the header of rbx_din.hip) with the deliberately wrong terms the host test needs."""
import torch

PAIR_NAMES = ("y", "dh", "dt", "dW", "db")
POOL_NAMES = ("weight", "out", "dscore", "dh")


def ref_pairs(h, t, w, b, act):
    tt = t.unsqueeze(1).expand(-1, h.shape[1], -1)
    pairs = torch.cat([tt, h, tt - h, tt * h], dim=-1)
    y = pairs.reshape(-1, pairs.shape[-1]) @ w.t()
    if b is not None:
        y = y + b
    return torch.relu(y) if act else y


def ref_pool(score, h, mask, softmax):
    w = score
    if mask is not None:
        w = w * mask
    if softmax:
        if mask is not None:
            w = w + -1.e9 * (1 - mask)
        w = w.softmax(dim=-1)
    return (w.unsqueeze(-1) * h).sum(dim=1)


# ---- cases: float32 values (what the kernels read), restated in either dtype ------------------------------------------------
def pairs_case(E, L, n, bias, seed, batch=37, up=1.0):
    """h [B, L, E], t [B, E], w [n, 4E], b [n] or None, r [B L, n]: the upstream gradient at std ``up`` (unit scale unless
    a test asks for a small one)."""
    g = torch.Generator().manual_seed(seed)
    return {"h": torch.randn(batch, L, E, generator=g), "t": torch.randn(batch, E, generator=g),
            "w": torch.randn(n, 4 * E, generator=g) * 0.3, "b": torch.randn(n, generator=g) * 0.3 if bias else None,
            "r": torch.randn(batch * L, n, generator=g) * up}


def pairs_preact(case):
    """The float64 pre-activation: a ReLU gate is decided by its sign."""
    return ref_pairs(case["h"].double(), case["t"].double(), case["w"].double(),
                     None if case["b"] is None else case["b"].double(), 0)


def pairs_reference(case, act, dtype=torch.float64):
    """{"y", "dh", "dt", "dW", "db"} through autograd over ref_pairs in ``dtype`` (db None without a bias)."""
    leaves = [None if case[k] is None else case[k].to(dtype).requires_grad_(True) for k in ("h", "t", "w", "b")]
    y = ref_pairs(leaves[0], leaves[1], leaves[2], leaves[3], act)
    grads = torch.autograd.grad((y * case["r"].to(dtype)).sum(), [x for x in leaves if x is not None])
    if leaves[3] is None:
        grads = tuple(grads) + (None,)
    return dict(zip(PAIR_NAMES, (y.detach(),) + tuple(grads)))


def pairs_manual(case, act, dtype=torch.float64, bug=None):
    """The backward of rbx_din.hip's header: dP = dy' W in four column blocks a..d, dh = dP_b - dP_c + dP_d o t,
    dt = sum_l (dP_a + dP_c + dP_d o h), dW = dy'^T [t, h, t - h, t o h], db = the column sums of dy'."""
    h, t, w, r = (case[k].to(dtype) for k in ("h", "t", "w", "r"))
    b = None if case["b"] is None else case["b"].to(dtype)
    B, L, E = h.shape
    y = ref_pairs(h, t, w, b, act)
    dy = r * (y > 0).to(dtype) if act else r
    dP = (dy @ w).reshape(B, L, 4, E)
    tt = t.unsqueeze(1).expand(-1, L, -1)
    dh = dP[:, :, 1] - dP[:, :, 2] + dP[:, :, 3] * tt
    c = dP[:, :, 2].clone()
    if bug == "dt without the last position of dP_c":
        c[:, L - 1] = 0
    dt = (dP[:, :, 0] + c + dP[:, :, 3] * h).sum(1)
    pairs = torch.cat([tt, h, tt - h, tt * h], dim=-1).reshape(B * L, 4 * E)
    rows = dy
    if bug == "db without the last row of a 1024-row split":
        rows = dy.clone()
        rows[min(B * L, 1024) - 1] = 0
    return {"y": y, "dh": dh, "dt": dt, "dW": dy.t() @ pairs, "db": rows.sum(0) if b is not None else None}


def pool_case(B, L, E, masking, seed, up=1.0, peak=0.0):
    """score [B, L], h [B, L, E], mask [B, L] or None, r [B, E].  masking: "none", "random" (70 % kept), "one_sample_all_masked"
    (sample min(3, B - 1) has no valid position), "fractions" (values in {0, 0.5, 1}: the kernels multiply by the mask, they do
    not select).  ``peak``: added to one score per sample (a peaked softmax)."""
    g = torch.Generator().manual_seed(seed)
    score = torch.randn(B, L, generator=g)
    h = torch.randn(B, L, E, generator=g)
    r = torch.randn(B, E, generator=g) * up
    mask = None
    if masking in ("random", "one_sample_all_masked"):
        mask = (torch.rand(B, L, generator=g) < 0.7).float()
        if masking == "one_sample_all_masked":
            mask[min(3, B - 1)] = 0.0
    elif masking == "fractions":
        mask = torch.randint(0, 3, (B, L), generator=g).float() * 0.5
        mask[torch.arange(B), torch.arange(B) % L] = 1.0         # (a valid position per sample: -1e9 / 2 is no fill to compare)
    elif masking != "none":
        raise ValueError(masking)
    if peak:
        score[torch.arange(B), torch.arange(B) % L] += peak
    return {"score": score, "h": h, "mask": mask, "r": r}


def small_pool_case():
    """The small-gradient case of tests/test_gpu_din_forms.py and tests/test_fp32_bar_host.py: L = 257 (one position past a
    stride of 256), upstream gradients of size 1e-3: dscore and dh are below 1e-3 everywhere."""
    return pool_case(37, 257, 16, "none", 77, up=1e-3)


def _pool_weight(score, mask, softmax):
    w = score if mask is None else score * mask
    if softmax:
        if mask is not None:
            w = w + -1.e9 * (1 - mask)
        w = w.softmax(dim=-1)
    return w


def pool_reference(case, softmax, dtype=torch.float64):
    """{"weight", "out", "dscore", "dh"} through autograd over ref_pool in ``dtype``."""
    score, h = (case[k].to(dtype).requires_grad_(True) for k in ("score", "h"))
    mask = None if case["mask"] is None else case["mask"].to(dtype)
    out = ref_pool(score, h, mask, softmax)
    ds, dh = torch.autograd.grad((out * case["r"].to(dtype)).sum(), (score, h))
    return {"weight": _pool_weight(score.detach(), mask, softmax), "out": out.detach(), "dscore": ds, "dh": dh}


def pool_manual(case, softmax, dtype=torch.float64, bug=None):
    """dw_l = <dout, h_l>; dscore = w (dw - sum_l w dw) o mask (softmax) or dw o mask; dh_l = w_l dout."""
    score, h, r = (case[k].to(dtype) for k in ("score", "h", "r"))
    mask = None if case["mask"] is None else case["mask"].to(dtype)
    w = _pool_weight(score, mask, softmax)
    out = (w.unsqueeze(-1) * h).sum(1)
    dw = torch.einsum("be,ble->bl", r, h)
    if softmax:
        dot = (w * dw).sum(1, keepdim=True)
        ds = w * dw if bug == "dscore without - dot" else w * (dw - dot)
    else:
        ds = dw
    if mask is not None:
        ds = ds * mask
    wh = w
    if bug == "dh of the last position under the weight before it" and w.shape[1] > 1:
        wh = w.clone()
        wh[:, -1] = w[:, -2]
    return {"weight": w, "out": out, "dscore": ds, "dh": wh.unsqueeze(-1) * r.unsqueeze(1)}
