"""Float64 restatement of the FM model body (LR + bias + second-order interaction) and of its gradients for a given
upstream gradient ``g = dL/dlogit``, with a bound per element.

For every output the restatement also returns ``A``, the same sum taken over absolute values, and the tests ask

    |got - want| <= C * eps32 * A + tiny

The bar follows from how the kernels sum, not from the order-free bound: float32 summation of n terms in sequence is only
bounded by about (n - 1) eps32 A, and a hot row sums tens of thousands of terms.  The kernels add a row's terms in a
shallow tree instead -- the forward's S over the F fields of a sample (F <= 52 here), a run of at most 40 sorted pairs per
lane group (tier B) or 16 per chunk (tier A), at most 32 chunk tails per lane group and step, 4 waves, then the steps of a
window walk and at most 16 workgroup partials (tier A: one partial per 2048-sample block, at most 32 blocks at B = 65 536)
-- each level a short sequential sum, so the rounding of a result is a few tens of eps32 times A at most.  C = 64 was the
starting value and was kept: the worst case measured stays below 4 % of the bar.  It is tight where few terms meet (a
row with one lookup) and grows with the hot rows, instead of a tolerance scaled by the largest entry of the tensor.  Rows
with ``A == 0`` (never looked up, padding rows) must come out exactly zero.

Model (the reference's FM: FeatureEmbedding -> InnerProductInteraction("product_sum") + LogisticRegression):
    e_f[b] = V_f[id_fb]        (categorical)      e_f[b] = x_fb * w_f        (numeric, x rounded to float32 first)
    l_f[b] = L_f[id_fb]                           l_f[b] = x_fb * wl_f
    S[b] = sum_f e_f[b],  logit[b] = sum_f l_f[b] + bias + 0.5 * sum_d (S^2 - sum_f e_f^2)
Gradients for g[b]:
    dV[id] += g (S - e_f)       dL[id] += g          (index_add over the lookups; padding rows stay zero)
    dw_f = sum_b g x (S - e_f)  dwl_f = sum_b g x    dbias = sum_b g
"""
import torch

EPS32 = float(torch.finfo(torch.float32).eps)
C_BOUND = 64            # one constant for every comparison against this restatement
TINY = 1e-30


class Table(object):
    """One parameter of the body in float64: ``weight`` is [V, D] (categorical, D = 1 for an LR table) or [D] / [] for a
    numeric feature's weight; ``pad`` the padding row or None.  Fields that share a table share the object."""

    def __init__(self, weight, pad=None):
        self.weight = weight.double()
        self.pad = pad


def fm_body64(fields, bias, g):
    """fields: list of (kind, column, emb_table, lr_table) with kind "categorical" (column: int64 ids [B]) or "numeric"
    (column: float64 values [B]); either table may be None.  bias: float64 scalar tensor or None.  g: float64 [B].
    Returns (logit, A_logit, grads, (dbias, A_dbias)) where grads maps id(Table) -> (Table, want, A)."""
    g = g.double().view(-1)
    B = g.shape[0]
    D = None
    for _, _, emb, _ in fields:
        if emb is not None:
            D = emb.weight.shape[-1]
            break
    ag = g.abs()

    def emb_of(kind, col, emb):
        if emb is None:
            return None
        if kind == "categorical":
            return emb.weight[col]
        return col[:, None] * emb.weight.view(1, -1)

    def lr_of(kind, col, lr):
        if lr is None:
            return None
        if kind == "categorical":
            return lr.weight.view(-1)[col]
        return col * lr.weight.view(())

    cols = []
    for kind, col, emb, lr in fields:
        if kind == "numeric":
            col = col.float().double()                  # the kernels (and the reference) read x as float32
        else:
            col = col.long()
        cols.append(col)
    S = torch.zeros(B, D or 1, dtype=torch.float64)
    Sa = torch.zeros_like(S)
    Q = torch.zeros_like(S)
    lin = torch.zeros(B, dtype=torch.float64)
    alin = torch.zeros_like(lin)
    for (kind, _, emb, lr), col in zip(fields, cols):
        e = emb_of(kind, col, emb)
        if e is not None:
            S += e
            Sa += e.abs()
            Q += e * e
        l1 = lr_of(kind, col, lr)
        if l1 is not None:
            lin += l1
            alin += l1.abs()
    b0 = bias.double().view(()) if bias is not None else torch.zeros((), dtype=torch.float64)
    logit = lin + b0
    a_logit = alin + b0.abs()
    if D is not None:
        logit = logit + 0.5 * (S * S - Q).sum(1)
        a_logit = a_logit + 0.5 * (Sa * Sa + Q).sum(1)
    grads = {}

    def acc(table, shape):
        ent = grads.get(id(table))
        if ent is None:
            ent = grads[id(table)] = (table, torch.zeros(shape, dtype=torch.float64), torch.zeros(shape, dtype=torch.float64))
        return ent

    for (kind, _, emb, lr), col in zip(fields, cols):
        if emb is not None:
            e = emb_of(kind, col, emb)
            de = g[:, None] * (S - e)
            ae = ag[:, None] * (Sa + e.abs())
            _, want, A = acc(emb, emb.weight.shape)
            if kind == "categorical":
                want.index_add_(0, col, de)
                A.index_add_(0, col, ae)
            else:
                want += (col[:, None] * de).sum(0).view(want.shape)
                A += (col.abs()[:, None] * ae).sum(0).view(A.shape)
        if lr is not None:
            _, want, A = acc(lr, lr.weight.shape)
            if kind == "categorical":
                want.view(-1).index_add_(0, col, g)
                A.view(-1).index_add_(0, col, ag)
            else:
                want += (g * col).sum().view(want.shape)
                A += (ag * col.abs()).sum().view(A.shape)
    for table, want, A in grads.values():
        if table.pad is not None:                       # nn.Embedding(padding_idx): the padding row gets no gradient
            want[table.pad] = 0
            A[table.pad] = 0
    return logit, a_logit, grads, (g.sum(), ag.sum())


def bound_ratio(got, want, A, C=C_BOUND):
    """max over the elements of |got - want| / (C eps32 A + tiny): <= 1 passes the bound."""
    got = got.detach().double().cpu().reshape(want.shape)
    err = (got - want).abs()
    return float((err / (C * EPS32 * A + TINY)).max()) if err.numel() else 0.0
