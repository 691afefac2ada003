"""rechub-style layers (drop-in for ``torch_rechub.basic.layers``,
/root/reference/recbox/third_party/rechub/basic/layers.py): ``EmbeddingLayer`` (+``InputMask``
and the three pooling modules), ``MLP``, ``FM``, ``LR``, ``PredictionLayer`` with the same
constructors, outputs, exceptions and parameter names (``embed_dict.<feature>.weight``,
``mlp.<i>.*``, ``fc.*``), ``FFM`` / ``CEN`` of DeepFFM / FatDeepFFM (``u``, ``mlp_att.*``), and the extractors of the
multi-interest and session models (``CapsuleNetwork``, ``MultiInterestSA``, ``GRU``).  ``EmbeddingLayer.forward`` is ONE ``rbx_embed_fwd`` launch for all
requested features: one-hot lookups, id-masked mean/sum pooling (mask = ``id != padding_idx``,
eps 1e-16, the pad row is a normal trainable row that just gets weight 0), concat pooling and
dense pass-through all land in one ``[B, width]`` row.
"""
import torch
import torch.nn as nn

from ... import _embed_host as host
from ... import dense, ops
from ..._lib import (FIELD_CATEGORICAL, FIELD_DENSE, POOL_CONCAT, POOL_MEAN_ID, POOL_NONE, POOL_SUM_ID)
from .features import DenseFeature, SequenceFeature, SparseFeature


class PredictionLayer(nn.Module):
    def __init__(self, task_type='classification'):
        super(PredictionLayer, self).__init__()
        if task_type not in ["classification", "regression"]:
            raise ValueError("task_type must be classification or regression")
        self.task_type = task_type

    def forward(self, x):
        return torch.sigmoid(x) if self.task_type == "classification" else x


class EmbeddingLayer(nn.Module):
    def __init__(self, features):
        super().__init__()
        self.features = features
        self.embed_dict = nn.ModuleDict()
        self.n_dense = 0
        self._plans = {}
        for fea in features:
            if fea.name in self.embed_dict:
                continue
            if isinstance(fea, SparseFeature) and fea.shared_with == None:  # noqa: E711
                self.embed_dict[fea.name] = fea.get_embedding_layer()
            elif isinstance(fea, SequenceFeature) and fea.shared_with == None:  # noqa: E711
                self.embed_dict[fea.name] = fea.get_embedding_layer()
            elif isinstance(fea, DenseFeature):
                self.n_dense += 1

    def _lookups(self, x, features):
        sparse, dense_l = [], []
        for fea in features:
            if isinstance(fea, DenseFeature):
                dense_l.append(host.Lookup(fea.name, FIELD_DENSE, None, 1))
                continue
            table = self.embed_dict[fea.name if fea.shared_with is None else fea.shared_with]
            if isinstance(fea, SparseFeature):
                sparse.append(host.Lookup(fea.name, FIELD_CATEGORICAL, table, table.embedding_dim))
            elif isinstance(fea, SequenceFeature):
                if fea.pooling not in ("sum", "mean", "concat"):
                    raise ValueError("Sequence pooling method supports only pooling in %s, got %s." %
                                     (["sum", "mean"], fea.pooling))
                pool = {"sum": POOL_SUM_ID, "mean": POOL_MEAN_ID, "concat": POOL_CONCAT}[fea.pooling]
                mask_id = fea.padding_idx if fea.padding_idx is not None else -1   # InputMask: id != -1
                sparse.append(host.Lookup(fea.name, FIELD_CATEGORICAL, table, table.embedding_dim, pool=pool,
                                          seq_len=x[fea.name].shape[1], mask_id=mask_id, eps=1e-16))
            else:
                raise ValueError("unknown feature class %s" % type(fea).__name__)
        return sparse, dense_l

    def _forward_with_bags(self, x, features, squeeze_dim):
        """Some sequence features arrive as ``ops.Bags`` (ragged indices / offsets) instead of ``[B, L]`` ids: they go
        through ``ops.embed_bags`` (rbx_embed_csr_*), every other feature through the usual plan (rbx_embed_fwd), and the
        slots are joined by columns in feature order.  Tables shared between the two calls get one gradient: the second
        backward node of the pass adds its rows into the first one's (ops.config.share_table_grads).  ``Bags`` that carry
        per-sample weights (pooling='sum' only) get an ``embed_bags`` call of their own, beside the unweighted ones'."""
        def weighted(f):
            return getattr(x[f.name], "weights", None) is not None

        key = ("bags", tuple(id(f) for f in features), squeeze_dim,
               tuple((("wbags" if weighted(f) else "bags") if isinstance(x[f.name], ops.Bags) else x[f.name].shape[1])
                     if isinstance(f, SequenceFeature) else 0 for f in features))
        cached = self._plans.get(key)
        if cached is None:
            order, padded = [], []
            specs, tables, offs = ([], []), ([], []), [0, 0]          # [0] the unweighted bags' call, [1] the weighted ones'
            for fea in features:
                if isinstance(fea, DenseFeature):
                    continue
                if not isinstance(x[fea.name], ops.Bags):
                    sparse, _ = self._lookups(x, [fea])
                    order.append(("padded", len(padded)))
                    padded += sparse
                    continue
                if not isinstance(fea, SequenceFeature):
                    raise ValueError("feature '%s': only a SequenceFeature takes ops.Bags" % fea.name)
                if fea.pooling == "concat":
                    raise ValueError("feature '%s': pooling='concat' keeps one slot per position; ragged ops.Bags need "
                                     "pooling 'sum' or 'mean'" % fea.name)
                if fea.pooling not in ("sum", "mean"):
                    raise ValueError("Sequence pooling method supports only pooling in %s, got %s." %
                                     (["sum", "mean"], fea.pooling))
                g = 1 if weighted(fea) else 0
                if g and fea.pooling == "mean":
                    raise NotImplementedError("feature '%s': per-sample weights go with pooling='sum' only; weighted mean "
                                              "pools are not implemented" % fea.name)
                table = self.embed_dict[fea.name if fea.shared_with is None else fea.shared_with]
                if not any(t is table for t in tables[g]):
                    tables[g].append(table)
                param = [i for i, t in enumerate(tables[g]) if t is table][0]
                mask_id = fea.padding_idx if fea.padding_idx is not None else -1   # InputMask: id != -1
                specs[g].append(ops.BagSpec(fea.name, table.embedding_dim, offs[g], param,
                                            POOL_SUM_ID if fea.pooling == "sum" else POOL_MEAN_ID, table.num_embeddings,
                                            padding_idx=table.padding_idx, mask_id=mask_id, eps=1e-16))
                order.append(("bags", (g, len(specs[g]) - 1)))
                offs[g] += table.embedding_dim
            n_sparse = len(order)
            if squeeze_dim:
                for fea in features:
                    if isinstance(fea, DenseFeature):
                        order.append(("padded", len(padded)))
                        padded.append(host.Lookup(fea.name, FIELD_DENSE, None, 1))
            cached = (host.Plan(padded) if padded else None, [ops.BagPlan(sp) if sp else None for sp in specs], tables, order,
                      n_sparse)
            self._plans[key] = cached
        plan, bag_plans, tables, order, n_sparse = cached
        out_p = plan.run([x[lk.name] for lk in plan.lookups]) if plan is not None else None
        out_b = [ops.embed_bags(bp, [x[s.name] for s in bp.specs], [t.weight for t in tb]) if bp is not None else None
                 for bp, tb in zip(bag_plans, tables)]
        pieces, dims, concat = [], set(), False
        for kind, i in order:
            if kind == "padded":
                sp = plan.specs[i]
                pieces.append(out_p[:, sp.out_off:sp.out_off + sp.width])
                concat = concat or sp.pool == POOL_CONCAT
                if sp.kind != FIELD_DENSE:
                    dims.add(sp.dim)
            else:
                sp = bag_plans[i[0]].specs[i[1]]
                pieces.append(out_b[i[0]][:, sp.out_off:sp.out_off + sp.dim])
                dims.add(sp.dim)
        out = torch.cat(pieces, 1)
        if squeeze_dim:
            return out
        if len(dims) != 1:
            raise RuntimeError("Sizes of tensors must match except in dimension 1 (embed_dim differs across features)")
        if concat:
            raise RuntimeError("Tensors must have same number of dimensions (mixing pooling='concat' "
                               "with pooled/sparse features)")
        return out.view(out.shape[0], n_sparse, dims.pop())

    def forward(self, x, features, squeeze_dim=False):
        if any(isinstance(x[f.name], ops.Bags) for f in features):
            return self._forward_with_bags(x, features, squeeze_dim)
        key = (tuple(id(f) for f in features), squeeze_dim,
               tuple(x[f.name].shape[1] if isinstance(f, SequenceFeature) else 0 for f in features))
        cached = self._plans.get(key)
        if cached is None:
            sparse, dense_l = self._lookups(x, features)
            if squeeze_dim:
                if not sparse and not dense_l:
                    raise ValueError("The input features can note be empty")
                lookups = sparse + dense_l                  # cat(sparse.flatten(1), dense_values)
            else:
                if not sparse:
                    raise ValueError(
                        "If keep the original shape:[batch_size, num_features, embed_dim], expected %s in feature "
                        "list, got %s" % ("SparseFeatures", features))
                lookups = sparse                            # dense values are dropped, as in the reference
            cached = (host.Plan(lookups), len(sparse))
            self._plans[key] = cached
        plan, n_sparse = cached
        # the flattened [B, sum(dims) + n_dense] layout rarely has 16-byte aligned rows (26 * 64 + 13 = 1677 floats):
        # it is produced with a padded row stride and consumed in place by the tower's first GEMM
        out = plan.run([x[lk.name] for lk in plan.lookups], pad_rows=squeeze_dim)
        if squeeze_dim:
            return out
        B = out.shape[0]
        specs = plan.specs
        if plan.uniform_dim is None:
            raise RuntimeError("Sizes of tensors must match except in dimension 1 (embed_dim differs across features)")
        concat = [s.pool == POOL_CONCAT for s in specs]
        if any(concat):
            if not all(concat) or len(set(s.seq_len for s in specs)) != 1:
                raise RuntimeError("Tensors must have same number of dimensions (mixing pooling='concat' "
                                   "with pooled/sparse features)")
            return out.view(B, n_sparse, specs[0].seq_len, plan.uniform_dim)
        return out.view(B, n_sparse, plan.uniform_dim)


class InputMask(nn.Module):
    """[B, n_features(, L)] float mask: id != padding_idx (or != -1 when no padding_idx)."""

    def forward(self, x, features):
        mask = []
        if not isinstance(features, list):
            features = [features]
        for fea in features:
            if isinstance(fea, SparseFeature) or isinstance(fea, SequenceFeature):
                pad = fea.padding_idx if fea.padding_idx != None else -1  # noqa: E711
                mask.append((x[fea.name].long() != pad).unsqueeze(1).float())
            else:
                raise ValueError("Only SparseFeature or SequenceFeature support to get mask.")
        return torch.cat(mask, dim=1)


class LR(nn.Module):
    def __init__(self, input_dim, sigmoid=False):
        super().__init__()
        self.sigmoid = sigmoid
        self.fc = nn.Linear(input_dim, 1, bias=True)

    def forward(self, x):
        y = ops.linear(x, self.fc.weight, self.fc.bias)
        return torch.sigmoid(y) if self.sigmoid else y


class ConcatPooling(nn.Module):
    def forward(self, x, mask=None):
        return x


class AveragePooling(nn.Module):
    """bmm(mask, x) / (mask.sum + 1e-16); plain mean over L when mask is None."""

    def forward(self, x, mask=None):
        if mask == None:  # noqa: E711
            return ops.pool(x, None, False, ops.DENOM_LEN, 0.0)
        return ops.pool(x, mask, True, ops.DENOM_MASK, 1e-16)


class SumPooling(nn.Module):
    def forward(self, x, mask=None):
        if mask == None:  # noqa: E711
            return ops.pool(x, None, False, ops.DENOM_NONE, 0.0)
        return ops.pool(x, mask, True, ops.DENOM_NONE, 0.0)


class Dice(nn.Module):
    """Dice activation (rechub/basic/activation.py:5-26), kept as written there."""

    def __init__(self, epsilon=1e-3):
        super(Dice, self).__init__()
        self.epsilon = epsilon
        self.alpha = nn.Parameter(torch.randn(1))

    def forward(self, x):
        avg = x.mean(dim=1).unsqueeze(dim=1)
        var = (torch.pow(x - avg, 2) + self.epsilon).sum(dim=1).unsqueeze(dim=1)
        ps = torch.sigmoid((x - avg) / torch.sqrt(var))
        return ps * x + (1 - ps) * self.alpha * x


def activation_layer(act_name):
    if isinstance(act_name, str):
        low = act_name.lower()
        if low == 'sigmoid':
            return nn.Sigmoid()
        if low == 'relu':
            return nn.ReLU(inplace=True)
        if low == 'dice':
            return Dice()
        if low == 'prelu':
            return nn.PReLU()
        if low == "softmax":
            return nn.Softmax(dim=1)
        raise NotImplementedError
    if issubclass(act_name, nn.Module):
        return act_name()
    raise NotImplementedError


class MLP(nn.Module):
    """Linear -> BatchNorm1d -> activation -> Dropout per layer (always BatchNorm), optional Linear(*,1)."""

    def __init__(self, input_dim, output_layer=True, dims=None, dropout=0, activation="relu"):
        super().__init__()
        if dims is None:
            dims = []
        layers = list()
        for i_dim in dims:
            layers.append(nn.Linear(input_dim, i_dim))
            layers.append(nn.BatchNorm1d(i_dim))
            layers.append(activation_layer(activation))
            layers.append(nn.Dropout(p=dropout))
            input_dim = i_dim
        if output_layer:
            layers.append(nn.Linear(input_dim, 1))
        self.mlp = nn.Sequential(*layers)

    def forward(self, x):
        return dense.run_sequential(self.mlp, x)


class FM(nn.Module):
    """0.5 * [(sum_f x)^2 - sum_f x^2], summed over embed_dim when reduce_sum."""

    def __init__(self, reduce_sum=True):
        super().__init__()
        self.reduce_sum = reduce_sum

    def forward(self, x):
        return ops.interaction(x, "product_sum" if self.reduce_sum else "bi_interaction")


class FFM(nn.Module):
    """Field-aware crosses of an already gathered block (rechub/basic/layers.py:651-682): x [B, F, F, D] ->
    x[:, i, j] * x[:, j, i] over the pairs i < j (i outer), [B, P, D], or its sum over D as [B, P, 1] with ``reduce_sum``.
    One indexed expression instead of the reference's P sliced multiplies and a stack.  This is NOT the hot path: the
    DeepFFM / FatDeepFFM mirrors never build the block, they call ``ops.ffm_cross`` on the raw ids."""

    def __init__(self, num_fields, reduce_sum=True):
        super().__init__()
        self.num_fields = num_fields
        self.reduce_sum = reduce_sum
        iu = torch.triu_indices(num_fields, num_fields, offset=1)
        self.register_buffer("_pair_i", iu[0].contiguous(), persistent=False)
        self.register_buffer("_pair_j", iu[1].contiguous(), persistent=False)

    def forward(self, x):
        crossed = x[:, self._pair_i, self._pair_j] * x[:, self._pair_j, self._pair_i]
        if self.reduce_sum:
            crossed = torch.sum(crossed, dim=-1, keepdim=True)
        return crossed


class CEN(nn.Module):
    """Compose-Excitation Network of FAT-DeepFFM (rechub/basic/layers.py:685-719): d = relu(sum_d u * em), s = mlp_att(d),
    out = (s[..., None] * em) flattened to [B, P * D].  The two FC layers run on the project's ``MLP``; the rescale is
    ``ops.row_scale`` where that op can be used -- its scale carries no gradient, so only when ``s`` needs none
    (inference).  There is no kernel of its own for the descriptor or the rescale."""

    def __init__(self, embed_dim, num_field_crosses, reduction_ratio):
        super().__init__()
        self.u = torch.nn.Parameter(torch.rand(num_field_crosses, embed_dim), requires_grad=True)
        self.mlp_att = MLP(num_field_crosses, dims=[num_field_crosses // reduction_ratio, num_field_crosses],
                           output_layer=False, activation="relu")

    def forward(self, em):
        d = torch.relu((self.u.squeeze(0) * em).sum(-1))
        s = self.mlp_att(d)
        if em.is_cuda and not (torch.is_grad_enabled() and s.requires_grad):
            aem = ops.row_scale(em, s)
        else:
            aem = s.unsqueeze(-1) * em
        return aem.flatten(start_dim=1)


class CapsuleNetwork(nn.Module):
    """The dynamic-routing capsule layer of MIND (``bilinear_type`` 0) and ComirecDR (``bilinear_type`` 2), layers.py:553-648
    of the reference: same constructor, parameter names (``linear.weight`` or ``w``, and the always-present
    ``relu.0.weight``) and ``forward(item_eb [B, L, D], mask [B, L]) -> [B, interest_num, D]``.  Types 0 and 1 transform with
    ``ops.linear``; type 2 with the per-position GEMMs of ``ops.capsule_bilinear_route``, so the ``[B, L, K D, D]`` product of
    the reference exists in neither pass; the routing iterations run on chip in one launch (``ops.capsule_route``).  Type 0
    draws its starting logits with exactly one ``torch.randn(B, K, L, device=...)`` call.

    Deliberate deviations: ``stop_grad`` is fixed to True as in the reference and setting it to False raises
    NotImplementedError at the next forward; the reference leaves ``w`` uninitialised (``torch.Tensor(...)``), here it is
    filled with N(0, 0.01^2) so that no kernel ever reads uninitialised memory."""

    def __init__(self, embedding_dim, seq_len, bilinear_type=2, interest_num=4, routing_times=3, relu_layer=False):
        super(CapsuleNetwork, self).__init__()
        self.embedding_dim = embedding_dim
        self.seq_len = seq_len
        self.bilinear_type = bilinear_type
        self.interest_num = interest_num
        self.routing_times = routing_times
        self.relu_layer = relu_layer
        self.stop_grad = True
        self.relu = nn.Sequential(nn.Linear(self.embedding_dim, self.embedding_dim, bias=False), nn.ReLU())
        if self.bilinear_type == 0:
            self.linear = nn.Linear(self.embedding_dim, self.embedding_dim, bias=False)
        elif self.bilinear_type == 1:
            self.linear = nn.Linear(self.embedding_dim, self.embedding_dim * self.interest_num, bias=False)
        else:
            self.w = nn.Parameter(torch.empty(1, self.seq_len, self.interest_num * self.embedding_dim,
                                              self.embedding_dim).normal_(0.0, 0.01))

    def forward(self, item_eb, mask):
        if not self.stop_grad:
            raise NotImplementedError("CapsuleNetwork: stop_grad=False (gradients through every routing iteration) is not "
                                      "implemented; the reference fixes it to True")
        B, L, D = item_eb.shape[0], self.seq_len, self.embedding_dim
        K, rt = self.interest_num, self.routing_times
        mask = mask.reshape(B, L)
        fused = ops.capsule_supported(L, D, K, rt, item_eb.dtype) and item_eb.is_cuda
        if not item_eb.is_cuda:
            ops._require_cuda(item_eb, "capsule input")
        init = None
        if self.bilinear_type == 0:
            hat = ops.linear(item_eb, self.linear.weight)                       # [B, L, D], shared by the interests
            init = torch.randn(B, K, L, device=item_eb.device)
        elif self.bilinear_type == 1:
            hat = ops.linear(item_eb, self.linear.weight)                       # [B, L, K D]
        elif fused:
            hat = None
        else:
            hat = ops.capsule_bilinear_torch(item_eb, self.w)
        if rt < 1:
            raise ValueError("CapsuleNetwork: routing_times=%d" % rt)
        if fused:
            if hat is None:
                out = ops.capsule_bilinear_route(item_eb, self.w, mask, K, rt)
            else:
                out = ops.capsule_route(hat, mask, K, rt, init=init, shared=self.bilinear_type == 0)
        else:
            out = ops.capsule_route_torch(hat, mask, K, rt, init=init, shared=self.bilinear_type == 0)
            if rt < 3:
                out = out.detach()
        if self.relu_layer:
            out = ops.linear(out, self.relu[0].weight, act="relu")
        return out


class MultiInterestSA(nn.Module):
    """The self-attentive multi-interest extractor of ComirecSA (layers.py:516-550 of the reference): same constructor,
    parameter names (``W1`` [D, H], ``W2`` [H, interest_num] and the unused ``W3`` [D, D]) and ``torch.rand`` init;
    ``forward(seq_emb [B, L, D], mask [B, L, 1] or [B, L] or None) -> [B, interest_num, D]`` is one ``ops.sa_pool`` call.  An explicit ``hidden_dim`` is honoured (the reference never sets
    the attribute in that case and fails in its constructor); the default is 4 D."""

    def __init__(self, embedding_dim, interest_num, hidden_dim=None):
        super(MultiInterestSA, self).__init__()
        self.embedding_dim = embedding_dim
        self.interest_num = interest_num
        self.hidden_dim = self.embedding_dim * 4 if hidden_dim is None else hidden_dim
        self.W1 = torch.nn.Parameter(torch.rand(self.embedding_dim, self.hidden_dim), requires_grad=True)
        self.W2 = torch.nn.Parameter(torch.rand(self.hidden_dim, self.interest_num), requires_grad=True)
        self.W3 = torch.nn.Parameter(torch.rand(self.embedding_dim, self.embedding_dim), requires_grad=True)

    def forward(self, seq_emb, mask=None):
        return ops.sa_pool(seq_emb, self.W1, self.W2, mask)[0]


class GRU(nn.Module):
    """What GRU4Rec (gru4rec.py:40-44) and NARM (narm.py:30) use of ``torch.nn.GRU``: ``input_size``, ``hidden_size``,
    ``num_layers``, ``bias``, ``batch_first``, with torch's parameter names (``weight_ih_l{k}``, ``weight_hh_l{k}``,
    ``bias_ih_l{k}``, ``bias_hh_l{k}``), shapes, gate order (r, z, n) and U(-1/sqrt(H), 1/sqrt(H)) init, so a reference
    checkpoint loads unchanged.  Each layer is one ``ops.gru`` call (input projection on the dense path, the recurrence as one
    launch).  ``forward(x, h0=None, lengths=None) -> (out, h_n [num_layers, B, H])``; ``lengths`` [B] (on the device) stands in
    for ``pack_padded_sequence`` / ``pad_packed_sequence``: positions at and beyond a sample's length are 0 in ``out`` and
    ``h_n`` is the state after its last valid step.  ``bidirectional``, ``dropout > 0`` and ``proj_size`` are not implemented."""

    def __init__(self, input_size, hidden_size, num_layers=1, bias=True, batch_first=False, dropout=0.0, bidirectional=False,
                 proj_size=0):
        super(GRU, self).__init__()
        if bidirectional or dropout > 0 or proj_size != 0:
            raise NotImplementedError("GRU: bidirectional, dropout > 0 and proj_size are not implemented")
        self.input_size, self.hidden_size, self.num_layers = input_size, hidden_size, num_layers
        self.bias, self.batch_first = bias, batch_first
        self.dropout, self.bidirectional, self.proj_size = 0.0, False, 0
        bound = 1.0 / hidden_size ** 0.5 if hidden_size > 0 else 0.0
        for k in range(num_layers):
            shapes = [("weight_ih_l%d" % k, (3 * hidden_size, input_size if k == 0 else hidden_size)),
                      ("weight_hh_l%d" % k, (3 * hidden_size, hidden_size))]
            if bias:
                shapes += [("bias_ih_l%d" % k, (3 * hidden_size,)), ("bias_hh_l%d" % k, (3 * hidden_size,))]
            for name, shape in shapes:
                setattr(self, name, nn.Parameter(torch.empty(*shape).uniform_(-bound, bound)))

    def forward(self, x, h0=None, lengths=None):
        if x.dim() != 3:
            raise NotImplementedError("GRU: the input must be [B, L, I] (batch_first) or [L, B, I]; packed and unbatched "
                                      "inputs are not implemented -- pass `lengths`")
        if not self.batch_first:
            x = x.transpose(0, 1).contiguous()
        finals = []
        for k in range(self.num_layers):
            x, h_n = ops.gru(x, getattr(self, "weight_ih_l%d" % k), getattr(self, "weight_hh_l%d" % k),
                             getattr(self, "bias_ih_l%d" % k) if self.bias else None,
                             getattr(self, "bias_hh_l%d" % k) if self.bias else None,
                             h0[k] if h0 is not None else None, lengths)
            finals.append(h_n)
        return (x if self.batch_first else x.transpose(0, 1)), torch.stack(finals, dim=0)


class SENETLayer(nn.Module):
    """FiBiNet's field gate (layers.py SENETLayer): ``mlp`` = Linear(F, R), ReLU, Linear(R, F), ReLU without biases,
    R = max(1, int(F / reduction_ratio)); parameters ``mlp.0.weight`` and ``mlp.2.weight``.  ``gate(x)`` [B, F] is one
    ``ops.senet_gate`` call; ``forward(x)`` returns ``x * gate(x)[..., None]`` as the reference does."""

    def __init__(self, num_fields, reduction_ratio=3):
        super(SENETLayer, self).__init__()
        reduced_size = max(1, int(num_fields / reduction_ratio))
        self.mlp = nn.Sequential(nn.Linear(num_fields, reduced_size, bias=False), nn.ReLU(),
                                 nn.Linear(reduced_size, num_fields, bias=False), nn.ReLU())

    def gate(self, x):
        return ops.senet_gate(x, self.mlp[0].weight, self.mlp[2].weight, "relu")

    def forward(self, x):
        return x * self.gate(x).unsqueeze(-1)


class BiLinearInteractionLayer(nn.Module):
    """FiBiNet's bilinear interaction (layers.py BiLinearInteractionLayer): ``bilinear_layer`` is one bias-free Linear(D, D)
    ('field_all': ``bilinear_layer.weight``) or a ModuleList of F ('field_each') or P = F (F - 1) / 2 ('field_interaction')
    of them (``bilinear_layer.<k>.weight``); any other type raises NotImplementedError.  ``forward(x)`` -> [B, P, D] is one
    ``ops.bilinear_pairs`` call over the stacked ``nn.Linear`` weights, read as [out, in]; ``forward(x, scale)`` -> [B, 2 P, D]
    appends the interaction of ``x * scale[..., None]`` (FiBiNet's second branch)."""

    def __init__(self, input_dim, num_fields, bilinear_type="field_interaction"):
        super(BiLinearInteractionLayer, self).__init__()
        self.bilinear_type = bilinear_type
        if self.bilinear_type == "field_all":
            self.bilinear_layer = nn.Linear(input_dim, input_dim, bias=False)
        elif self.bilinear_type == "field_each":
            self.bilinear_layer = nn.ModuleList([nn.Linear(input_dim, input_dim, bias=False) for _ in range(num_fields)])
        elif self.bilinear_type == "field_interaction":
            self.bilinear_layer = nn.ModuleList([nn.Linear(input_dim, input_dim, bias=False)
                                                 for _ in range(num_fields * (num_fields - 1) // 2)])
        else:
            raise NotImplementedError()

    def stacked_weight(self):
        """[M, D, D]: the matrices as ``nn.Linear`` stores them ([out, in])."""
        if self.bilinear_type == "field_all":
            return self.bilinear_layer.weight.unsqueeze(0)
        return torch.stack([m.weight for m in self.bilinear_layer], dim=0)

    def forward(self, x, scale=None):
        return ops.bilinear_pairs(x, self.stacked_weight(), self.bilinear_type, transposed=True, scale=scale)


def _project(x, layer):
    """``layer(x)`` for a bias-free nn.Linear: the dense GEMM on the GPU, the module itself for CPU tensors."""
    return ops.linear(x, layer.weight) if x.is_cuda else layer(x)


def _cross(x0, xi, h, bias):
    """``xi + x0 * h + bias``: one pass (``ops.cross``) on the GPU."""
    return ops.cross(x0, xi, h, bias) if x0.is_cuda else x0 * h + bias + xi


class CrossLayer(nn.Module):
    """One DCN cross term without its residual (layers.py CrossLayer, used by EDCN): ``w(x_i) * x_0 + b`` with ``w`` a bias-free
    Linear(input_dim, 1) and ``b`` [input_dim].  ``residual(x_0, x_i)`` is ``x_i + forward(x_0, x_i)`` in one pass."""

    def __init__(self, input_dim):
        super(CrossLayer, self).__init__()
        self.w = torch.nn.Linear(input_dim, 1, bias=False)
        self.b = torch.nn.Parameter(torch.zeros(input_dim))

    def forward(self, x_0, x_i):
        return _project(x_i, self.w) * x_0 + self.b

    def residual(self, x_0, x_i):
        return _cross(x_0, x_i, _project(x_i, self.w), self.b)


class CrossNetwork(nn.Module):
    """DCN's cross network (layers.py CrossNetwork): ``x = x0 * w_i(x) + b_i + x`` per layer, ``w`` a ModuleList of bias-free
    Linear(input_dim, 1), ``b`` a ParameterList of [input_dim]; over ``ops.linear`` + ``ops.cross``."""

    def __init__(self, input_dim, num_layers):
        super().__init__()
        self.num_layers = num_layers
        self.w = torch.nn.ModuleList([torch.nn.Linear(input_dim, 1, bias=False) for _ in range(num_layers)])
        self.b = torch.nn.ParameterList([torch.nn.Parameter(torch.zeros((input_dim,))) for _ in range(num_layers)])

    def forward(self, x):
        x0 = x
        for i in range(self.num_layers):
            x = _cross(x0, x, _project(x, self.w[i]), self.b[i])
        return x


class CrossNetV2(nn.Module):
    """DCN-V2's full-rank cross network (layers.py CrossNetV2): ``x = x0 * w_i(x) + b_i + x`` with ``w`` bias-free
    Linear(input_dim, input_dim) and a separate ``b``; over ``ops.linear`` + ``ops.cross``."""

    def __init__(self, input_dim, num_layers):
        super().__init__()
        self.num_layers = num_layers
        self.w = torch.nn.ModuleList([torch.nn.Linear(input_dim, input_dim, bias=False) for _ in range(num_layers)])
        self.b = torch.nn.ParameterList([torch.nn.Parameter(torch.zeros((input_dim,))) for _ in range(num_layers)])

    def forward(self, x):
        x0 = x
        for i in range(self.num_layers):
            x = _cross(x0, x, _project(x, self.w[i]), self.b[i])
        return x


class CrossNetMix(nn.Module):
    """DCN-V2's mixture of low-rank cross experts (layers.py CrossNetMix): per layer ``u_list`` / ``v_list`` [experts, input_dim,
    low_rank], ``c_list`` [experts, low_rank, low_rank] (xavier-normal) and ``bias`` [input_dim, 1]; ``gating`` is one bias-free
    Linear(input_dim, 1) per expert, shared by the layers.  The stack is one ``ops.cross_mix`` call.  The reference ends with
    ``x_l.squeeze()``, so a batch of one returns [input_dim]; so does this."""

    def __init__(self, input_dim, num_layers=2, low_rank=32, num_experts=4):
        super(CrossNetMix, self).__init__()
        self.num_layers = num_layers
        self.num_experts = num_experts
        self.u_list = torch.nn.ParameterList([nn.Parameter(nn.init.xavier_normal_(
            torch.empty(num_experts, input_dim, low_rank))) for i in range(self.num_layers)])
        self.v_list = torch.nn.ParameterList([nn.Parameter(nn.init.xavier_normal_(
            torch.empty(num_experts, input_dim, low_rank))) for i in range(self.num_layers)])
        self.c_list = torch.nn.ParameterList([nn.Parameter(nn.init.xavier_normal_(
            torch.empty(num_experts, low_rank, low_rank))) for i in range(self.num_layers)])
        self.gating = nn.ModuleList([nn.Linear(input_dim, 1, bias=False) for i in range(self.num_experts)])
        self.bias = torch.nn.ParameterList([nn.Parameter(nn.init.zeros_(
            torch.empty(input_dim, 1))) for i in range(self.num_layers)])

    def forward(self, x):
        gate_w = torch.cat([g.weight for g in self.gating], dim=0)                     # [E, input_dim]
        x_l = ops.cross_mix(x, list(self.u_list), list(self.v_list), list(self.c_list), gate_w, list(self.bias))
        return x_l.unsqueeze(2).squeeze()
