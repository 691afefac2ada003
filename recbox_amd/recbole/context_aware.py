"""The interaction parts of RecBole's AFM, AutoInt and FiGNN (third_party/recbole/model/context_aware_recommender/afm.py,
autoint.py, fignn.py)."""
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


class GraphLayer(nn.Module):
    """``GraphLayer`` of fignn.py:29-50: the parameters ``W_in``, ``W_out`` [num_fields, embedding_size, embedding_size]
    (Xavier normal) and ``bias_p`` [embedding_size] (zeros) of one message-passing layer.  ``forward(g [B, F, F], h [B, F, A])
    -> a [B, F, A]`` is the reference's; ``FiGNNInteraction`` never calls it -- a whole layer is one ``ops.fignn_step``."""

    def __init__(self, num_fields, embedding_size):
        super(GraphLayer, self).__init__()
        self.W_in = nn.Parameter(torch.Tensor(num_fields, embedding_size, embedding_size))
        self.W_out = nn.Parameter(torch.Tensor(num_fields, embedding_size, embedding_size))
        xavier_normal_(self.W_in)
        xavier_normal_(self.W_out)
        self.bias_p = nn.Parameter(torch.zeros(embedding_size))

    def forward(self, g, h):
        h_out = torch.einsum("fnk,bfk->bfn", self.W_out, h)
        return torch.einsum("fnk,bfk->bfn", self.W_in, torch.bmm(g, h_out)) + self.bias_p


class FiGNNInteraction(nn.Module):
    """``FiGNN.fignn_layer`` (third_party/recbole/model/context_aware_recommender/fignn.py:107-144) with the parameters it
    reads, under the reference model's attribute names: ``att_embedding``, ``self_attn`` (a real
    ``nn.MultiheadAttention(batch_first=True)``, never called), ``v_res_embedding``, ``gnn`` (``n_layers - 1`` ``GraphLayer``s),
    ``W_attn``, ``gru_cell`` (a real ``nn.GRUCell``, never called), ``mlp1``, ``mlp2`` and ``dropout_layer``; the
    ``state_dict`` keys are the reference's.

    ``fignn_layer(in_feature [B, F, D]) -> [B, 1]`` (= ``forward``): ``ops.linear``, then ONE ``ops.field_attn`` with the
    residual ``v_res_embedding(in_feature)`` and the relu in its epilogue, then ``n_layers - 1`` x ``ops.fignn_step`` (edge
    weights, GraphLayer, GRU cell and ``+ att_feature`` as one launch each way; the first also writes ``self.graph``
    [B, F, F]), then the attentional scoring ``sum_f mlp2(h)_f * mlp1(h)_f``.  ``n_layers = 1`` skips the steps, as the
    reference does.  ``attn_dropout`` drops attention probabilities only in ``self.training``.  The embedding tables and the
    loss are not part of this module."""

    def __init__(self, num_feature_field, embedding_size, attention_size, n_layers, num_heads, hidden_dropout_prob=0.0,
                 attn_dropout_prob=0.0):
        super(FiGNNInteraction, self).__init__()
        if n_layers < 1:
            raise ValueError("FiGNNInteraction: n_layers = %d" % n_layers)
        self.num_feature_field = num_feature_field
        self.embedding_size = embedding_size
        self.attention_size = attention_size
        self.n_layers = n_layers
        self.num_heads = num_heads
        self.hidden_dropout_prob = hidden_dropout_prob
        self.attn_dropout_prob = attn_dropout_prob
        self.dropout_layer = nn.Dropout(p=hidden_dropout_prob)
        self.att_embedding = nn.Linear(embedding_size, attention_size)
        self.self_attn = nn.MultiheadAttention(attention_size, num_heads, dropout=attn_dropout_prob, batch_first=True)
        self.v_res_embedding = nn.Linear(embedding_size, attention_size)
        self.gnn = nn.ModuleList([GraphLayer(num_feature_field, attention_size) for _ in range(n_layers - 1)])
        self.leaky_relu = nn.LeakyReLU(negative_slope=0.01)
        self.W_attn = nn.Linear(attention_size * 2, 1, bias=False)
        self.gru_cell = nn.GRUCell(attention_size, attention_size)
        self.mlp1 = nn.Linear(attention_size, 1, bias=False)
        self.mlp2 = nn.Linear(num_feature_field * attention_size, num_feature_field, bias=False)
        self.graph = None
        self.apply(self._init_weights)

    def _init_weights(self, module):
        """Xavier-normal weights for every Embedding and Linear, zero Linear biases (fignn.py:146-155); the GRU cell keeps
        torch's own init, as in the reference (whose last branch tests for ``nn.GRU``)."""
        if isinstance(module, (nn.Embedding, nn.Linear)):
            xavier_normal_(module.weight.data)
            if getattr(module, "bias", None) is not None:
                constant_(module.bias.data, 0)

    @staticmethod
    def _linear(m, x):
        return ops.linear(x, m.weight, m.bias) if x.is_cuda else m(x)

    def fignn_layer(self, in_feature):
        if (in_feature.dim() != 3 or in_feature.shape[1] != self.num_feature_field
                or in_feature.shape[2] != self.embedding_size):
            raise RuntimeError("FiGNNInteraction: in_feature %s is not [B, %d, %d]"
                               % (tuple(in_feature.shape), self.num_feature_field, self.embedding_size))
        F, A = self.num_feature_field, self.attention_size
        emb_feature = self.dropout_layer(self._linear(self.att_embedding, in_feature))         # [B, F, A]
        attn = self.self_attn
        att_feature, _ = ops.field_attn(emb_feature, attn.in_proj_weight, attn.in_proj_bias, attn.out_proj.weight,
                                        attn.out_proj.bias, self.num_heads,
                                        residual=self._linear(self.v_res_embedding, in_feature), relu=True,
                                        dropout_p=self.attn_dropout_prob if self.training else 0.0)
        w_attn = self.W_attn.weight[0]
        cell = self.gru_cell
        h = att_feature
        if self.n_layers > 1:
            for i, layer in enumerate(self.gnn):
                h, graph = ops.fignn_step(h, att_feature, w_attn, layer.W_out, layer.W_in, layer.bias_p, cell.weight_ih,
                                          cell.weight_hh, cell.bias_ih, cell.bias_hh, want_graph=(i == 0))
                if i == 0:
                    self.graph = graph
        else:                                                                                  # the graph alone
            s, d = att_feature.detach() @ w_attn[:A], att_feature.detach() @ w_attn[A:]
            alpha = self.leaky_relu(s.unsqueeze(2) + d.unsqueeze(1))
            alpha = alpha.masked_fill(torch.eye(F, dtype=torch.bool, device=alpha.device), float("-inf"))
            self.graph = torch.softmax(alpha, dim=-1).detach()
        score = self._linear(self.mlp1, h).squeeze(-1)                                         # [B, F]
        weight = self._linear(self.mlp2, h.flatten(start_dim=1))                               # [B, F]
        return (weight * score).sum(dim=1).unsqueeze(-1)                                       # [B, 1]

    def forward(self, in_feature):
        return self.fignn_layer(in_feature)
