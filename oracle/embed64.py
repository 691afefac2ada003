"""Float64 restatement of the generic embedding lookup (rbx_embed_fwd / rbx_embed_bwd: every EmbeddingLayer,
FeatureEmbedding and rechub EmbeddingLayer call) and of its gradients for a given upstream gradient ``dY [B, width]``,
with a bound per element, in the conventions of oracle/fm64.py:

    |got - want| <= C * eps32 * A + tiny          A: the same sum taken over absolute values

and ``A == 0`` (rows no lookup reached, padding rows, rows only masked ids named) means exactly zero.

Definitions (oracle/recbox_oracle.c, orc_embed_fwd / orc_embed_bwd, and the kernels' comments); a lookup writes the
``width`` columns of the output row that start at its ``out_off``:
    dense        out = float32(x)                                                      no parameter
    numeric      out = float32(x) * w                       dw  = sum_b x_b dY[b]
    categorical, ids [B, L], rows r_bl = W[id_bl]:
      NONE       out = r_b0                                 (L = 1)
      CONCAT     out[l] = r_bl                              dW[id_bl] += dY[b, l]
      SUM        out = sum_l r_bl                           dW[id_bl] += dY[b]
      SUM_ID     out = sum_l k_bl r_bl, k = (id != mask_id) dW[id_bl] += k_bl dY[b]
      MEAN_ID    out = s_b sum_l k_bl r_bl                  dW[id_bl] += s_b k_bl dY[b],  s_b = 1 / (sum_l k_bl + eps)
      MEAN_VALUE out = s_b sum_l r_bl                       dW[id_bl] += s_b dY[b],       s_b = 1 / (#{l: sum_d r_bl != 0} + eps)
    The row a lookup's descriptor names as ``padding_idx`` gets no gradient from THAT lookup (the forward reads it like
    any other row); ``eps`` is the float32 the descriptor carries.  Lookups that share a table share the ``Table``
    object and one gradient.  MEAN_VALUE's mask is decided on the float64 rows: callers keep every row either all zeros
    or with a row sum well away from zero (``assert_value_mask_is_safe``), so that float32 agrees.

Constants.  Backward: C = C_BOUND, the constant of fm64.py, whose argument is about the sorted reduce's tree (a run of at
most 40 sorted pairs per lane group, at most 32 chunk tails per lane group and step, 4 waves, the steps of a window walk,
at most 16 workgroup partials): the generic lookup runs that same code.  Mean pooling multiplies a term by the forward's
float32 ``row_scale`` (within 1 ulp of the float64 reciprocal: 2 eps32 A at most), inside the constant.  Forward: a
sample's pool is a sum of at most L rows and one scaling, so C = max(C_BOUND, L + 2): the order-free bound where
histories are longer than the constant covers, the project's constant otherwise.  One-id lookups, CONCAT and dense
columns are copies: C = 0 there, the output must be equal.
"""
import numpy as np
import torch

from oracle.fm64 import C_BOUND, EPS32, TINY, Table, bound_ratio  # noqa: F401  (one set of conventions for both files)

POOLS = ("NONE", "SUM", "MEAN_VALUE", "MEAN_ID", "SUM_ID", "CONCAT")


class Lookup64(object):
    """One output slot.  kind: "categorical" (column: ids [B] or [B, L], any dtype; truncated like .long()), "numeric"
    or "dense" (column: values [B]); table: a ``Table`` ([V, D] rows, or [D] for a numeric weight; None for dense)."""

    def __init__(self, kind, column, table=None, dim=1, pool="NONE", seq_len=1, padding_idx=None, mask_id=None, eps=0.0,
                 out_off=0):
        assert pool in POOLS and kind in ("categorical", "numeric", "dense")
        self.kind, self.column, self.table, self.dim, self.pool = kind, column, table, int(dim), pool
        self.seq_len, self.padding_idx, self.mask_id, self.out_off = int(seq_len), padding_idx, mask_id, int(out_off)
        self.eps = float(np.float32(eps))

    @property
    def width(self):
        return self.dim * (self.seq_len if self.pool == "CONCAT" else 1)

    @property
    def terms(self):
        """Rows that one output element sums (the forward's order-free constant is terms + 2)."""
        return self.seq_len if self.pool in ("SUM", "SUM_ID", "MEAN_ID", "MEAN_VALUE") else 1


def _pieces(lk, B):
    """(ids [B, L], rows [B, L, D], keep [B, L], scale [B]) of a categorical lookup, all float64 / int64."""
    ids = lk.column.long().reshape(B, lk.seq_len)
    rows = lk.table.weight[ids]
    keep = torch.ones(ids.shape, dtype=torch.float64)
    if lk.pool in ("SUM_ID", "MEAN_ID") and lk.mask_id is not None:
        keep = (ids != lk.mask_id).double()
    scale = torch.ones(B, dtype=torch.float64)
    if lk.pool == "MEAN_ID":
        scale = 1.0 / (keep.sum(1) + lk.eps)
    elif lk.pool == "MEAN_VALUE":
        scale = 1.0 / ((rows.sum(2) != 0).double().sum(1) + lk.eps)
    return ids, rows, keep, scale


def embed64(lookups, dY, width=None, counts=None):
    """Returns (out, A_out, C_out, grads): out / A_out float64 [B, width]; C_out [width], the forward's constant per
    column (0: a copy, must be equal); grads maps id(Table) -> (Table, want, A).  ``counts``: a dict that receives the
    number of non-zero terms behind every element, under "out" and under id(Table) (what a sequential float32 sum's own
    bound is stated in), and under ("scaled", ...) of the same keys whether a mean pool's scale or a numeric feature's value multiplied one of them."""
    dY = dY.double()
    B = dY.shape[0]
    width = dY.shape[1] if width is None else width
    out = torch.zeros(B, width, dtype=torch.float64)
    a_out = torch.zeros_like(out)
    c_out = torch.zeros(width, dtype=torch.float64)
    grads = {}
    n_out = torch.zeros_like(out)
    s_out = torch.zeros_like(out)

    def acc(table):
        ent = grads.get(id(table))
        if ent is None:
            shape = table.weight.shape
            ent = grads[id(table)] = (table, torch.zeros(shape, dtype=torch.float64), torch.zeros(shape, dtype=torch.float64))
            if counts is not None:
                counts[id(table)] = torch.zeros(shape, dtype=torch.float64)
                counts["scaled", id(table)] = torch.zeros(shape, dtype=torch.float64)
        return ent

    for lk in lookups:
        sl = slice(lk.out_off, lk.out_off + lk.width)
        g = dY[:, sl]
        if lk.kind == "dense":
            out[:, lk.out_off] = lk.column.float().double().view(B)
            a_out[:, lk.out_off] = out[:, lk.out_off].abs()
            continue
        if lk.kind == "numeric":
            x = lk.column.float().double().view(B)                # the kernels (and the reference) read x as float32
            w = lk.table.weight.view(-1)
            out[:, sl] = x[:, None] * w
            a_out[:, sl] = out[:, sl].abs()
            c_out[sl] = C_BOUND
            _, want, A = acc(lk.table)
            want += (x[:, None] * g).sum(0).view(want.shape)
            A += (x.abs()[:, None] * g.abs()).sum(0).view(A.shape)
            n_out[:, sl] = 1
            s_out[:, sl] = 1
            if counts is not None:
                counts[id(lk.table)] += ((x[:, None] * g) != 0).double().sum(0).view(A.shape)
                counts["scaled", id(lk.table)] += 1
            continue
        L, D = lk.seq_len, lk.dim
        ids, rows, keep, scale = _pieces(lk, B)
        if lk.pool == "NONE":
            assert L == 1
            out[:, sl] = rows[:, 0]
            a_out[:, sl] = rows[:, 0].abs()
            gl = g.reshape(B, 1, D)
            n_out[:, sl] = 1
        elif lk.pool == "CONCAT":
            out[:, sl] = rows.reshape(B, L * D)
            a_out[:, sl] = out[:, sl].abs()
            gl = g.reshape(B, L, D)
            n_out[:, sl] = 1
        else:
            out[:, sl] = (rows * keep[:, :, None]).sum(1) * scale[:, None]
            a_out[:, sl] = (rows.abs() * keep[:, :, None]).sum(1) * scale[:, None]
            c_out[sl] = max(C_BOUND, L + 2)
            gl = g.reshape(B, 1, D).expand(B, L, D)
            n_out[:, sl] = ((rows * keep[:, :, None]) != 0).double().sum(1)
            s_out[:, sl] = 1.0 if lk.pool in ("MEAN_ID", "MEAN_VALUE") else 0.0
        wgt = keep * scale[:, None]
        if lk.padding_idx is not None:
            wgt = wgt * (ids != lk.padding_idx).double()
        _, want, A = acc(lk.table)
        contrib = (wgt[:, :, None] * gl).reshape(B * L, D)
        want.index_add_(0, ids.reshape(-1), contrib)
        A.index_add_(0, ids.reshape(-1), contrib.abs())
        if counts is not None:
            counts[id(lk.table)].index_add_(0, ids.reshape(-1), (contrib != 0).double())
            if lk.pool in ("MEAN_ID", "MEAN_VALUE"):
                counts["scaled", id(lk.table)].index_add_(0, ids.reshape(-1), (contrib != 0).double())
    if counts is not None:
        counts["out"], counts["scaled", "out"] = n_out, s_out
    return out, a_out, c_out, grads


def forward_ratio(got, want, A, C):
    """max over the elements of |got - want| / (C eps32 A + tiny) with a constant per column; columns with C == 0 are
    copies: any difference there returns inf."""
    got = got.detach().double().cpu().reshape(want.shape)
    err = (got - want).abs()
    if err.numel() == 0:
        return 0.0
    copies = C == 0
    if bool(copies.any()) and float(err[:, copies].max()) != 0.0:
        return float("inf")
    return float((err / (C.view(1, -1) * EPS32 * A + TINY))[:, ~copies].max()) if bool((~copies).any()) else 0.0


def assert_value_mask_is_safe(weight):
    """MEAN_VALUE counts rows whose sum over d is not zero: float32 (any summation order) and float64 agree when every row
    either is all zeros or has |row sum| > 1e-3 (float32 rounding of a sum of D <= 1024 entries below 1 stays under 1e-4)."""
    w = weight.double()
    s = w.sum(-1).abs()
    zero = (w == 0).all(-1)
    bad = ~zero & (s <= 1e-3)
    assert not bool(bad.any()), "%d rows with a row sum within 1e-3 of zero" % int(bad.sum())
