"""Field-aware FM restated in torch float64 on the CPU (helper of the FFM tests, not a test).

Field i owns a table of ``vocab_i * F`` rows; id x names the block of rows ``x * F .. x * F + F - 1``.  The cross of the
pair i < j (i outer, j inner) is the row field i keeps for field j times the row field j keeps for field i.  DeepFFM
sums a first-order table per feature, runs an MLP over the flattened crosses, adds a bias and squashes; FatDeepFFM
rescales every cross by a per-pair attention first (descriptor = relu of the cross's inner product with a learned
vector, attention = two Linear + BatchNorm + ReLU layers over the descriptors)."""
import torch


def pairs(F):
    return [(i, j) for i in range(F - 1) for j in range(i + 1, F)]


def gather_blocks(tables, ids):
    """[B, F, F, D]: entry [b, i, j] is row x_i(b) * F + j of table i."""
    F = len(tables)
    return torch.stack([t.reshape(-1, F, t.shape[1])[x.long()] for t, x in zip(tables, ids)], dim=1)


def cross(tables, ids, reduce_sum=False):
    """[B, P, D] (or [B, P]) in the dtype of the tables (float64 for the bound, float32 for the exact forward)."""
    E = gather_blocks(tables, ids)
    out = torch.stack([E[:, i, j] * E[:, j, i] for i, j in pairs(len(tables))], dim=1)
    return out.sum(-1) if reduce_sum else out


def make_case(F, D, batch, seed=0, blocks=None, std=1.0, up=1.0):
    """{"tables": F x [blocks_i * F, D], "ids": F x [B], "r": {False: [B, P, D], True: [B, P]} (the upstream gradients of the
    Hadamard and the summed form, at std ``up``)} in float32 on the CPU."""
    g = torch.Generator().manual_seed(1000 * F + D + seed)
    blocks = blocks if blocks is not None else [1 + (7 * i + 3 * F) % 50 for i in range(F)]          # 1 .. 50 blocks
    P = F * (F - 1) // 2
    return {"tables": [torch.randn(nb * F, D, generator=g) * std for nb in blocks],
            "ids": [torch.randint(0, nb, (batch,), generator=g) for nb in blocks],
            "r": {False: torch.randn(batch, P, D, generator=g) * up, True: torch.randn(batch, P, generator=g) * up}}


def small_mult_case():
    """The small-gradient case of tests/test_gpu_ffm_forms.py and tests/test_fp32_bar_host.py: runs of thousands of equal keys,
    tables at std 1e-3 (an embedding early in training) and upstream gradients of size 1e-3."""
    return make_case(5, 16, 6181, seed=2, blocks=[1, 3, 1, 3, 3], std=1e-3, up=1e-3)


def small_wide_case():
    """D = 128 (the generic form, 32 float4s per row) with the same small tables and gradients."""
    return make_case(5, 128, 37, seed=1, std=1e-3, up=1e-3)


def reference(case, reduce_sum, dtype=torch.float64):
    """(out, [dtable_i]) of ``cross`` through autograd in ``dtype``: float64 for the bound, float32 (the ``*_ref32`` twin)
    for the bar of tests/fp32_bar.py."""
    ts = [t.to(dtype).requires_grad_(True) for t in case["tables"]]
    out = cross(ts, case["ids"], reduce_sum)
    grads = torch.autograd.grad(out, ts, case["r"][bool(reduce_sum)].to(dtype))
    return out.detach(), list(grads)


def reference32(case, reduce_sum):
    return reference(case, reduce_sum, torch.float32)


def manual(case, reduce_sum, dtype=torch.float64, bug=None):
    """(out, [dtable_i]) with the backward written out: dE[b, i, j] = dout[b, p(i, j)] o E[b, j, i], summed into block x_i(b)
    of table i.  ``bug``: "dtable 0 without its last sample" (one contribution of a run is lost), "dot product without the
    last float4" (reduce_sum only)."""
    tables = [t.to(dtype) for t in case["tables"]]
    ids, r = case["ids"], case["r"][bool(reduce_sum)].to(dtype)
    F, D = len(tables), tables[0].shape[1]
    E = gather_blocks(tables, ids)
    prod = torch.stack([E[:, i, j] * E[:, j, i] for i, j in pairs(F)], dim=1)
    if reduce_sum:
        out = (prod[..., :D - 4] if bug == "dot product without the last float4" else prod).sum(-1)
    else:
        out = prod
    dE = torch.zeros_like(E)
    for p, (i, j) in enumerate(pairs(F)):
        g = r[:, p].unsqueeze(-1) if reduce_sum else r[:, p]
        dE[:, i, j] = g * E[:, j, i]
        dE[:, j, i] = g * E[:, i, j]
    grads = []
    for i, (t, x) in enumerate(zip(tables, ids)):
        keep = slice(0, len(x) - 1) if (bug == "dtable 0 without its last sample" and i == 0) else slice(None)
        grads.append(torch.zeros(t.shape[0] // F, F, D, dtype=dtype).index_add_(0, x.long()[keep], dE[keep, i]).reshape(t.shape))
    return out, grads


def _mlp(sd, prefix, x, training=True, eps=1e-5):
    """rechub's MLP: Linear -> BatchNorm1d (batch statistics in training mode) -> ReLU -> Dropout(0) per hidden layer, then
    an optional Linear(*, 1); the layers are found by their state_dict keys ``<prefix>mlp.<k>.*``."""
    k = 0
    while True:
        w = sd.get("%smlp.%d.weight" % (prefix, k))
        if w is None:
            return x
        if w.dim() == 2:
            x = x @ w.t() + sd["%smlp.%d.bias" % (prefix, k)]
            k += 1
            continue
        if training:
            mean, var = x.mean(0), x.var(0, unbiased=False)
        else:
            mean, var = sd["%smlp.%d.running_mean" % (prefix, k)], sd["%smlp.%d.running_var" % (prefix, k)]
        x = (x - mean) / torch.sqrt(var + eps) * w + sd["%smlp.%d.bias" % (prefix, k)]
        x = torch.relu(x)
        k += 3                                               # BatchNorm, activation, Dropout


def deepffm_forward(sd, x, linear_names, cross_names, fat=False):
    """``sd``: a float64 state_dict (tensors that require grad where a gradient is wanted); ``x``: {name: [B] ids}."""
    y_lin = sum(sd["linear_embedding.embed_dict.%s.weight" % n][x[n].long()] for n in linear_names).sum(1, keepdim=True)
    tables = [sd["ffm_embedding.embed_dict.%s.weight" % n] for n in cross_names]
    em = cross(tables, [x[n] for n in cross_names])
    if fat:
        d = torch.relu((sd["cen.u"] * em).sum(-1))
        s = _mlp(sd, "cen.mlp_att.", d)
        em = s.unsqueeze(-1) * em
    y = y_lin + _mlp(sd, "mlp_out.", em.flatten(1))
    return torch.sigmoid(y.squeeze(1) + sd["b"])
