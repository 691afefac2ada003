"""``recbox_amd.bag.EmbeddingBag``: ``torch.nn.EmbeddingBag`` over the ragged (CSR) lookup, a thin ``nn.Module`` around
``ops.embed_bags`` -- the mapping INTEGRATION.md ("An ``nn.EmbeddingBag`` caller") gives, made once."""
import torch
from torch import nn

from . import ops

_POOL = {"sum": (ops.POOL_SUM, ops.POOL_SUM_ID), "mean": (ops.POOL_MEAN_ID, ops.POOL_MEAN_ID), "max": (ops.POOL_MAX, ops.POOL_MAX)}
# eps of mode="mean": the smallest normal float32, 2^-126.  count + eps rounds to count for every count >= 1, so a
# non-empty bag is bit-equal to eps = 0, and 1 / eps is finite, so an empty bag is 0 * (1 / eps) = torch's zero row.
# (Anything smaller is subnormal: whether it survives depends on the denormal mode, and below 2^-128 its reciprocal is inf.)
MEAN_EPS = 2.0 ** -126


class EmbeddingBag(nn.Module):
    """``nn.EmbeddingBag(num_embeddings, embedding_dim, mode=..., padding_idx=..., include_last_offset=...)`` on the GPU
    through ``ops.embed_bags``; ``forward(input, offsets=None, per_sample_weights=None)`` as torch's.

    * ``mode``: "sum" -> POOL_SUM, "mean" -> POOL_MEAN_ID, "max" -> POOL_MAX; with ``padding_idx=p`` the id ``p`` is left
      out of the sum, the count, the max and the gradient (``mask_id=p, padding_idx=p``; "sum" then runs as POOL_SUM_ID).
    * "mean" divides by ``count + MEAN_EPS`` with ``MEAN_EPS = 2^-126``, the smallest eps that leaves every non-empty bag
      bit-equal to ``eps = 0`` and gives an empty bag torch's zero row.  An empty bag is a zero row in every mode.
    * 1-D ``input`` takes ``offsets`` (int32 / int64, on the device); without ``include_last_offset`` the end
      ``input.numel()`` is appended with ``torch.cat``: no sync.  2-D ``[B, L]`` input is ``B`` bags of ``L`` ids:
      ``offsets = arange(0, B * L + 1, L)`` on the device, and ``offsets`` must be None.
    * ``per_sample_weights``: float32, the shape of ``input``, "sum" only (torch's rule); it may require a gradient.
    * ``max_norm``, ``scale_grad_by_freq`` and ``sparse`` are not implemented (the gradient is dense and deterministic;
      ``recbox_amd.optim`` steps the touched rows only)."""

    def __init__(self, num_embeddings, embedding_dim, max_norm=None, norm_type=2.0, scale_grad_by_freq=False, mode="mean",
                 sparse=False, _weight=None, include_last_offset=False, padding_idx=None):
        super().__init__()
        if max_norm is not None:
            raise NotImplementedError("recbox_amd.bag.EmbeddingBag: max_norm is not implemented")
        if scale_grad_by_freq:
            raise NotImplementedError("recbox_amd.bag.EmbeddingBag: scale_grad_by_freq is not implemented")
        if sparse:
            raise NotImplementedError("recbox_amd.bag.EmbeddingBag: sparse gradients are not implemented; the dense gradient "
                                      "is written on the touched rows only (recbox_amd.optim steps those)")
        if mode not in _POOL:
            raise ValueError("mode has to be one of sum, mean or max, got %r" % (mode,))
        if padding_idx is not None:
            if not -num_embeddings <= padding_idx < num_embeddings:
                raise ValueError("padding_idx must be within num_embeddings")
            padding_idx = padding_idx % num_embeddings
        self.num_embeddings, self.embedding_dim, self.mode = num_embeddings, embedding_dim, mode
        self.padding_idx, self.include_last_offset = padding_idx, include_last_offset
        if _weight is None:
            self.weight = nn.Parameter(torch.empty(num_embeddings, embedding_dim))
            nn.init.normal_(self.weight)
            if padding_idx is not None:
                with torch.no_grad():
                    self.weight[padding_idx].fill_(0)
        else:
            if tuple(_weight.shape) != (num_embeddings, embedding_dim):
                raise ValueError("shape of _weight does not match num_embeddings and embedding_dim")
            self.weight = nn.Parameter(_weight)
        pool = _POOL[mode][0 if padding_idx is None else 1]
        spec = ops.BagSpec("bag", embedding_dim, 0, 0, pool, num_embeddings, padding_idx=padding_idx, mask_id=padding_idx,
                           eps=MEAN_EPS if mode == "mean" else 0.0)
        self._plan = ops.BagPlan([spec])

    def forward(self, input, offsets=None, per_sample_weights=None):
        if per_sample_weights is not None:
            if self.mode != "sum":
                raise NotImplementedError("embedding_bag: per_sample_weights was not None. per_sample_weights is only "
                                          "supported for mode='sum' (got mode='%s')" % self.mode)
            if tuple(per_sample_weights.shape) != tuple(input.shape):
                raise ValueError("embedding_bag: per_sample_weights must have the shape of input, got %s and %s"
                                 % (tuple(per_sample_weights.shape), tuple(input.shape)))
        if input.dim() == 2:
            if offsets is not None:
                raise ValueError("if input is 2D, then offsets has to be None, as input is treated as a mini-batch of "
                                 "fixed length sequences")
            B, L = input.shape
            offsets = torch.arange(0, B * L + 1, L, dtype=torch.int64, device=input.device) if L > 0 else \
                torch.zeros(B + 1, dtype=torch.int64, device=input.device)
            input = input.reshape(-1)
            if per_sample_weights is not None:
                per_sample_weights = per_sample_weights.reshape(-1)
        elif input.dim() == 1:
            if offsets is None:
                raise ValueError("offsets has to be a 1D Tensor but got None")
            if offsets.dim() != 1:
                raise ValueError("offsets has to be a 1D Tensor")
            if not self.include_last_offset:
                end = torch.full((1,), input.numel(), dtype=offsets.dtype, device=offsets.device)
                offsets = torch.cat([offsets, end])
        else:
            raise ValueError("input has to be 1D or 2D Tensor, but got Tensor of dimension %d" % input.dim())
        return ops.embed_bags(self._plan, [ops.Bags(input, offsets, per_sample_weights)], [self.weight])

    def extra_repr(self):
        s = "%d, %d, mode=%r" % (self.num_embeddings, self.embedding_dim, self.mode)
        if self.padding_idx is not None:
            s += ", padding_idx=%d" % self.padding_idx
        return s
