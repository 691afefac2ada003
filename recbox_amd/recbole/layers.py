"""``AttLayer`` of RecBole (third_party/recbole/model/layers.py:236-261)."""
import torch
from torch import nn


class AttLayer(nn.Module):
    """The attention signal of a 3-D input: ``softmax_M(sum_A relu(x W^T) * h)``.  ``infeatures`` [B, M, in_dim] -> [B, M].
    The reference's constructor and ``state_dict`` keys (``w.weight`` [att_dim, in_dim], ``h`` [att_dim]).  This general form
    has no pair structure to exploit, so it runs the composition on any device; AFM's use of it over the field pairs is
    ``ops.afm_pool`` (``context_aware.AFMInteraction``), which reads these two parameters."""

    def __init__(self, in_dim, att_dim):
        super(AttLayer, self).__init__()
        self.in_dim = in_dim
        self.att_dim = att_dim
        self.w = nn.Linear(in_features=in_dim, out_features=att_dim, bias=False)
        self.h = nn.Parameter(torch.randn(att_dim), requires_grad=True)

    def forward(self, infeatures):
        att_signal = torch.relu(self.w(infeatures))                    # [B, M, att_dim]
        att_signal = torch.sum(torch.mul(att_signal, self.h), dim=2)   # [B, M]
        return torch.softmax(att_signal, dim=1)
