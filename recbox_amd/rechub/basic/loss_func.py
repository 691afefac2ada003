"""Pair-wise losses (drop-in for ``torch_rechub.basic.loss_func``: ``HingeLoss``, ``BPRLoss``)."""
import torch

from ... import ops


class HingeLoss(torch.nn.Module):
    """``mean(max(max(neg_score, -1) - pos_score + margin, 0))``; with ``num_items`` every term is weighted by
    ``log(rank + 1)``, rank = the share of negatives inside the margin times ``num_items``.  The reference takes ``torch.mean``
    of the bool tensor of those negatives, which raises in current torch; the share is formed in the scores' dtype here."""

    def __init__(self, margin=2, num_items=None):
        super().__init__()
        self.margin = margin
        self.n_items = num_items

    def forward(self, pos_score, neg_score):
        loss = torch.maximum(torch.max(neg_score, dim=-1).values - pos_score + self.margin, torch.tensor([0]).type_as(pos_score))
        if self.n_items is not None:
            impostors = neg_score - pos_score.view(-1, 1) + self.margin > 0
            rank = torch.mean(impostors.type_as(pos_score), -1) * self.n_items
            return torch.mean(loss * torch.log(rank + 1))
        return torch.mean(loss)


class BPRLoss(torch.nn.Module):
    """``mean(-log sigmoid(pos_score - neg_score), dim=-1)``.  One score per pair on the GPU -- the result is a scalar -- is
    ``ops.pair_logsigmoid_loss`` (one pass each way, fixed-order sum) on d = pos - neg: -(logsigmoid(d) + logsigmoid(-(-d))) is
    twice the term, so the scale is 0.5 / N.  Scores of more dimensions (a mean per row) and CPU tensors keep the reference's
    expression."""

    def __init__(self):
        super().__init__()

    def forward(self, pos_score, neg_score):
        if (pos_score.is_cuda and pos_score.dim() == 1 and pos_score.shape == neg_score.shape and pos_score.numel() > 0
                and pos_score.dtype == torch.float32 and neg_score.dtype == torch.float32):
            d = pos_score - neg_score
            return ops.pair_logsigmoid_loss(d, -d, None, 0.5 / d.numel())
        return torch.mean(-(pos_score - neg_score).sigmoid().log(), dim=-1)
