"""The interaction part of RecBole's AFM (third_party/recbole/model/context_aware_recommender/afm.py)."""
import torch
from torch import nn
from torch.nn.init import constant_, xavier_normal_

from .. import ops
from .layers import AttLayer


class AFMInteraction(nn.Module):
    """``AFM.afm_layer`` (afm.py:75-99) with the parameters it reads, under the reference model's attribute names: ``attlayer``
    (``AttLayer(embedding_size, attention_size)``), ``p`` [embedding_size] and ``dropout_layer``.  Its ``state_dict`` keys
    ``attlayer.w.weight``, ``attlayer.h`` and ``p`` load from the entries of a RecBole AFM checkpoint.

    ``forward(feat_emb [B, F, D]) -> [B, 1]``: ``ops.afm_pool`` (one launch each way on the GPU; nothing of [B, P, D] or
    [B, P, A] is formed), then dropout, the product with ``p`` and the sum over D.  The embedding tables, the first-order term
    and the loss of the reference model are not part of this module."""

    def __init__(self, num_feature_field, embedding_size, attention_size, dropout_prob):
        super(AFMInteraction, self).__init__()
        self.num_feature_field = num_feature_field
        self.embedding_size = embedding_size
        self.attention_size = attention_size
        self.dropout_prob = dropout_prob
        self.num_pair = num_feature_field * (num_feature_field - 1) / 2
        self.attlayer = AttLayer(embedding_size, attention_size)
        self.p = nn.Parameter(torch.randn(embedding_size), requires_grad=True)
        self.dropout_layer = nn.Dropout(p=dropout_prob)
        self.apply(self._init_weights)

    def _init_weights(self, module):
        """Xavier-normal weights for every Embedding and Linear, zero Linear biases (afm.py:45-51); ``h`` and ``p`` keep their
        standard normal draw."""
        if isinstance(module, (nn.Embedding, nn.Linear)):
            xavier_normal_(module.weight.data)
            if getattr(module, "bias", None) is not None:
                constant_(module.bias.data, 0)

    def attention(self, feat_emb):
        """The attention weights over the pairs [B, P] (detached), row-major pair order."""
        return ops.afm_pool(feat_emb, self.attlayer.w.weight, self.attlayer.h, want_attn=True)[1]

    def forward(self, feat_emb):
        if feat_emb.dim() != 3 or feat_emb.shape[1] != self.num_feature_field or feat_emb.shape[2] != self.embedding_size:
            raise RuntimeError("AFMInteraction: feat_emb %s is not [B, %d, %d]"
                               % (tuple(feat_emb.shape), self.num_feature_field, self.embedding_size))
        att_pooling, _ = ops.afm_pool(feat_emb, self.attlayer.w.weight, self.attlayer.h)      # [B, D]
        att_pooling = self.dropout_layer(att_pooling)
        att_pooling = torch.mul(att_pooling, self.p)
        return torch.sum(att_pooling, dim=1, keepdim=True)                                     # [B, 1]

    def reg_loss(self, reg_weight):
        """``reg_weight * ||attlayer.w.weight||_2`` (afm.py:115)."""
        return reg_weight * torch.norm(self.attlayer.w.weight, p=2)
