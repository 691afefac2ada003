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
