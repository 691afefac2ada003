"""The interaction parts of RecBole's AFM and AutoInt (third_party/recbole/model/context_aware_recommender/afm.py, autoint.py)."""
import torch
from torch import nn
from torch.nn.init import constant_, xavier_normal_

from .. import ops
from .layers import AttLayer, MLPLayers


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


class AutoIntInteraction(nn.Module):
    """``AutoInt.autoint_layer`` (third_party/recbole/model/context_aware_recommender/autoint.py:78-103) with the parameters it
    reads, under the reference model's attribute names: ``att_embedding``, ``mlp_layers``, ``self_attns`` (a ``ModuleList`` of
    real ``nn.MultiheadAttention``, so the ``state_dict`` keys ``self_attns.<i>.in_proj_weight`` ... and ``_init_weights``
    agree), ``attn_fc``, ``deep_predict_layer``, ``v_res_embedding`` (only with ``has_residual``) and ``dropout_layer``.

    ``forward(infeature [B, F, D]) -> [B, 1]``: the attention modules are never called -- every layer is one ``ops.field_attn``
    launch each way on their parameters, with the batch kept in front (the reference's two transposes disappear); the last
    call carries the residual ``v_res_embedding(infeature)`` and the relu.  ``dropout_probs[0]`` drops attention probabilities
    only in ``self.training``; ``dropout_probs[1]`` is the MLP's; ``dropout_probs[2]`` belongs to ``dropout_layer``, which the
    reference builds and never applies.  The embedding tables, the first-order term and the loss are not part of this module."""

    def __init__(self, num_feature_field, embedding_size, attention_size, n_layers, num_heads, mlp_hidden_size, dropout_probs,
                 has_residual):
        super(AutoIntInteraction, self).__init__()
        if n_layers < 1:
            raise ValueError("AutoIntInteraction: n_layers = %d (the residual and the relu ride the last layer)" % n_layers)
        self.num_feature_field = num_feature_field
        self.embedding_size = embedding_size
        self.attention_size = attention_size
        self.dropout_probs = list(dropout_probs)
        self.n_layers = n_layers
        self.num_heads = num_heads
        self.mlp_hidden_size = list(mlp_hidden_size)
        self.has_residual = has_residual
        self.att_embedding = nn.Linear(self.embedding_size, self.attention_size)
        self.embed_output_dim = self.num_feature_field * self.embedding_size
        self.atten_output_dim = self.num_feature_field * self.attention_size
        self.mlp_layers = MLPLayers([self.embed_output_dim] + self.mlp_hidden_size, dropout=self.dropout_probs[1])
        self.self_attns = nn.ModuleList([nn.MultiheadAttention(self.attention_size, self.num_heads, dropout=self.dropout_probs[0])
                                         for _ in range(self.n_layers)])
        self.attn_fc = nn.Linear(self.atten_output_dim, 1)
        self.deep_predict_layer = nn.Linear(self.mlp_hidden_size[-1], 1)
        if self.has_residual:
            self.v_res_embedding = nn.Linear(self.embedding_size, self.attention_size)
        self.dropout_layer = nn.Dropout(p=self.dropout_probs[2])
        self.apply(self._init_weights)

    def _init_weights(self, module):
        """Xavier-normal weights for every Embedding and Linear, zero Linear biases (autoint.py:70-76); this reaches the
        attention modules' ``out_proj`` but not their ``in_proj_weight``, as in the reference."""
        if isinstance(module, (nn.Embedding, nn.Linear)):
            xavier_normal_(module.weight.data)
            if getattr(module, "bias", None) is not None:
                constant_(module.bias.data, 0)

    @staticmethod
    def _linear(m, x):
        return ops.linear(x, m.weight, m.bias) if x.is_cuda else m(x)

    def forward(self, infeature):
        if infeature.dim() != 3 or infeature.shape[1] != self.num_feature_field or infeature.shape[2] != self.embedding_size:
            raise RuntimeError("AutoIntInteraction: infeature %s is not [B, %d, %d]"
                               % (tuple(infeature.shape), self.num_feature_field, self.embedding_size))
        batch_size = infeature.shape[0]
        cross_term = self._linear(self.att_embedding, infeature)                              # [B, F, A]
        p = self.dropout_probs[0] if self.training else 0.0
        last = len(self.self_attns) - 1
        for i, attn in enumerate(self.self_attns):
            res = self._linear(self.v_res_embedding, infeature) if (self.has_residual and i == last) else None
            cross_term, _ = ops.field_attn(cross_term, attn.in_proj_weight, attn.in_proj_bias, attn.out_proj.weight,
                                           attn.out_proj.bias, self.num_heads, residual=res, relu=(i == last), dropout_p=p)
        cross_term = cross_term.reshape(batch_size, self.atten_output_dim)
        deep = self._linear(self.deep_predict_layer, self.mlp_layers(infeature.reshape(batch_size, -1)))
        return self._linear(self.attn_fc, cross_term) + deep                                  # [B, 1]
