"""Mirrors of RecBole's graph collaborative-filtering networks (third_party/recbole/model/general_recommender) over
``ops.graph_prop`` / ``ops.graph_prop_mean`` (the ``torch.sparse.mm`` composition; no kernel: DESIGN.md): ``norm_adj`` (``get_norm_adj_mat`` of lightgcn.py /
ngcf.py on the device), ``LightGCNEncoder`` (lightgcn.py:60-151), ``BiGNNLayer`` (model/layers.py:208-233), ``NGCFEncoder``
(ngcf.py:50-165) and the losses of model/loss.py, ``BPRLoss``, ``RegLoss`` (Caser's) and ``EmbLoss``.  RecBole's ``(config,
dataset)`` constructors, ``GeneralRecommender``, ``calculate_loss`` and the trainers are not mirrored: an encoder takes the
sizes and the graph."""
import torch
from torch import nn

from .. import ops


def norm_adj(n_users, n_items, user_ids, item_ids, segment=None):
    """The symmetric normalised adjacency D^-0.5 A D^-0.5 of the bipartite interaction graph over n_users + n_items nodes
    (``get_norm_adj_mat``), as an ``ops.PropGraph`` on the device of the ids.  A repeated interaction counts once, as in the
    reference's ``dok`` dict; degrees come from the deduplicated matrix.  The values follow the reference's chain: d^-0.5 of
    (degree + 1e-7) in float64, ``(d_i^-0.5 * 1) * d_j^-0.5`` in float64, rounded once to float32."""
    u, i = user_ids.reshape(-1).long(), item_ids.reshape(-1).long()
    if u.numel() != i.numel():
        raise ValueError("norm_adj: %d user ids, %d item ids" % (u.numel(), i.numel()))
    if u.numel() and (int(u.min()) < 0 or int(u.max()) >= n_users or int(i.min()) < 0 or int(i.max()) >= n_items):
        raise ValueError("norm_adj: an id lies outside %d users x %d items" % (n_users, n_items))
    pair = torch.unique(u * n_items + i)
    u, i = torch.div(pair, n_items, rounding_mode="floor"), pair % n_items
    deg = torch.cat([torch.bincount(u, minlength=n_users), torch.bincount(i, minlength=n_items)])
    dinv = (deg.double() + 1e-7).pow(-0.5)
    rows, cols = torch.cat([u, i + n_users]), torch.cat([i + n_users, u])
    vals = ((dinv[rows] * 1.0) * dinv[cols]).float()
    n = n_users + n_items
    return ops.PropGraph.from_coo(rows, cols, vals, (n, n), segment)


class BPRLoss(nn.Module):
    """``-log(gamma + sigmoid(pos - neg)).mean()`` (loss.py:21-47).  One float32 score per pair on the GPU is
    ``ops.pair_logsigmoid_loss`` on d = pos - neg (twice the term, so the scale is 0.5 / N), which is the reference's value
    to within gamma = 1e-10 relative to sigmoid(d); anything else keeps the reference's expression."""

    def __init__(self, gamma=1e-10):
        super(BPRLoss, self).__init__()
        self.gamma = gamma

    def forward(self, pos_score, neg_score):
        if (pos_score.is_cuda and pos_score.dim() == 1 and pos_score.shape == neg_score.shape and pos_score.numel() > 0
                and pos_score.dtype == torch.float32 and neg_score.dtype == torch.float32):
            d = pos_score - neg_score
            return ops.pair_logsigmoid_loss(d, -d, None, 0.5 / d.numel())
        return -torch.log(self.gamma + torch.sigmoid(pos_score - neg_score)).mean()


class RegLoss(nn.Module):
    """L2 regularisation on model parameters (loss.py:50-63): the sum of the 2-norms of the tensors given; ``None`` for none."""

    def forward(self, parameters):
        reg_loss = None
        for W in parameters:
            reg_loss = W.norm(2) if reg_loss is None else reg_loss + W.norm(2)
        return reg_loss


class EmbLoss(nn.Module):
    """Regularisation on embeddings (loss.py:66-88): the sum of the p-norms (``require_pow``: of their p-th powers, over p)
    over the batch size of the last one; shape [1] as in the reference."""

    def __init__(self, norm=2):
        super(EmbLoss, self).__init__()
        self.norm = norm

    def forward(self, *embeddings, require_pow=False):
        emb_loss = torch.zeros(1, device=embeddings[-1].device)
        for e in embeddings:
            n = torch.norm(e, p=self.norm)
            emb_loss = emb_loss + (torch.pow(n, self.norm) if require_pow else n)
        emb_loss = emb_loss / embeddings[-1].shape[0]
        return emb_loss / self.norm if require_pow else emb_loss


class LightGCNEncoder(nn.Module):
    """The network of ``recbole.model.general_recommender.lightgcn.LightGCN``: ``user_embedding.weight`` and
    ``item_embedding.weight`` (``xavier_uniform_``), and ``forward() -> (user_all, item_all)``, the mean over the layers
    0 .. n_layers of the propagated tables, through ``ops.graph_prop_mean`` with the two tables passed as a pair.  ``graph`` is
    the ``ops.PropGraph`` of ``norm_adj``."""

    def __init__(self, n_users, n_items, embedding_size, n_layers, graph):
        super(LightGCNEncoder, self).__init__()
        if tuple(graph.shape) != (n_users + n_items, n_users + n_items):
            raise ValueError("LightGCNEncoder: the graph is %s, expected %d nodes" % (graph.shape, n_users + n_items))
        self.n_users, self.n_items, self.latent_dim, self.n_layers = n_users, n_items, embedding_size, n_layers
        self.user_embedding = nn.Embedding(n_users, embedding_size)
        self.item_embedding = nn.Embedding(n_items, embedding_size)
        nn.init.xavier_uniform_(self.user_embedding.weight)
        nn.init.xavier_uniform_(self.item_embedding.weight)
        self.graph = graph
        self.restore_user_e = None
        self.restore_item_e = None

    def _apply(self, fn, *args, **kwargs):
        out = super(LightGCNEncoder, self)._apply(fn, *args, **kwargs)
        dev = self.user_embedding.weight.device
        if self.graph.device != dev:
            self.graph = self.graph.to(dev)
        return out

    def forward(self):
        if self.training:
            self.restore_user_e, self.restore_item_e = None, None
        tables = (self.user_embedding.weight, self.item_embedding.weight)
        if self.n_layers == 0:
            return tables
        return ops.graph_prop_mean(self.graph, tables, self.n_layers)

    def full_sort_predict(self, user):
        """[B, n_items] scores of every item for the users ``user``; the propagated tables are kept until the next
        training forward."""
        if self.restore_user_e is None or self.restore_item_e is None:
            with torch.no_grad():
                self.restore_user_e, self.restore_item_e = self.forward()
        return ops.linear(self.restore_user_e[user], self.restore_item_e)


class BiGNNLayer(nn.Module):
    """``(L + I) E W_1 + (L E * E) W_2`` (model/layers.py:208-233) with the reference's keys ``linear.*`` and
    ``interActTransform.*``: ``L E`` is ``ops.graph_prop``, the two Linears are ``ops.linear``.  ``forward(graph,
    features, edge_scale=None)``: the eye matrix of the reference is not needed, ``edge_scale`` is the node dropout."""

    def __init__(self, in_dim, out_dim):
        super(BiGNNLayer, self).__init__()
        self.in_dim, self.out_dim = in_dim, out_dim
        self.linear = nn.Linear(in_features=in_dim, out_features=out_dim)
        self.interActTransform = nn.Linear(in_features=in_dim, out_features=out_dim)

    def forward(self, graph, features, edge_scale=None):
        x = ops.graph_prop(graph, features, edge_scale=edge_scale)
        lin = ops.linear if features.is_cuda else nn.functional.linear
        part1 = lin(features + x, self.linear.weight, self.linear.bias)
        part2 = lin(x * features, self.interActTransform.weight, self.interActTransform.bias)
        return part1 + part2


class NGCFEncoder(nn.Module):
    """The network of ``recbole.model.general_recommender.ngcf.NGCF`` (ngcf.py:50-165): ``user_embedding``, ``item_embedding``
    and ``GNNlayers.<k>.*`` (``xavier_normal_`` weights, zero biases, as ``xavier_normal_initialization``), LeakyReLU 0.2,
    message dropout (``ops.dropout``), ``ops.l2_normalize`` and the layer outputs concatenated along the width.  Node dropout
    is a per-edge scale ``floor(rand + keep) / keep`` drawn once per forward, as ``SparseDropout`` draws it (layers.py:1614):
    a dropped edge is a zero factor instead of a rebuilt matrix."""

    def __init__(self, n_users, n_items, embedding_size, hidden_size_list, graph, node_dropout=0.0, message_dropout=0.1):
        super(NGCFEncoder, self).__init__()
        if tuple(graph.shape) != (n_users + n_items, n_users + n_items):
            raise ValueError("NGCFEncoder: the graph is %s, expected %d nodes" % (graph.shape, n_users + n_items))
        self.n_users, self.n_items = n_users, n_items
        self.hidden_size_list = [embedding_size] + list(hidden_size_list)
        self.node_dropout, self.message_dropout = node_dropout, message_dropout
        self.user_embedding = nn.Embedding(n_users, embedding_size)
        self.item_embedding = nn.Embedding(n_items, embedding_size)
        self.GNNlayers = nn.ModuleList(BiGNNLayer(a, b) for a, b in zip(self.hidden_size_list[:-1], self.hidden_size_list[1:]))
        for m in self.modules():
            if isinstance(m, (nn.Embedding, nn.Linear)):
                nn.init.xavier_normal_(m.weight)
                if isinstance(m, nn.Linear) and m.bias is not None:
                    nn.init.constant_(m.bias, 0)
        self.graph = graph

    def _apply(self, fn, *args, **kwargs):
        out = super(NGCFEncoder, self)._apply(fn, *args, **kwargs)
        dev = self.user_embedding.weight.device
        if self.graph.device != dev:
            self.graph = self.graph.to(dev)
        return out

    def edge_scale(self):
        """The node dropout of this forward as a per-edge factor, or None."""
        if not self.training or self.node_dropout == 0:
            return None
        keep = 1.0 - self.node_dropout
        return torch.floor(torch.rand(self.graph.nnz, device=self.graph.device) + keep) * (1.0 / keep)

    def forward(self):
        scale = self.edge_scale()
        h = torch.cat([self.user_embedding.weight, self.item_embedding.weight], dim=0)
        outs = [h]
        for gnn in self.GNNlayers:
            h = gnn(self.graph, h, scale)
            h = nn.functional.leaky_relu(h, negative_slope=0.2)
            if h.is_cuda:
                h = ops.l2_normalize(ops.dropout(h, self.message_dropout, self.training))
            else:
                h = nn.functional.normalize(nn.functional.dropout(h, self.message_dropout, self.training), p=2, dim=1)
            outs.append(h)
        return torch.split(torch.cat(outs, dim=1), [self.n_users, self.n_items])
