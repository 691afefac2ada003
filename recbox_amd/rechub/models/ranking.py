"""DeepFM (drop-in for ``torch_rechub.models.ranking.DeepFM``,
/root/reference/recbox/third_party/rechub/models/ranking/deepfm.py:14-42), DIN with its ActivationUnit
(``torch_rechub.models.ranking.din``, rechub/models/ranking/din.py:16-91), and DeepFFM / FatDeepFFM
(``torch_rechub.models.ranking.deepffm``, rechub/models/ranking/deepffm.py:15-123), FiBiNet, and the Deep & Cross family: DCN,
DCNv2, EDCN with its BridgeModule / RegulationModule, and WideDeep (rechub/models/ranking/dcn.py, dcn_v2.py, edcn.py,
widedeep.py)."""
import torch

from ... import dense, ops
from ..basic.features import DenseFeature, SparseFeature
from ..basic.layers import (CEN, FFM, FM, LR, MLP, BiLinearInteractionLayer, CrossLayer, CrossNetMix, CrossNetV2, CrossNetwork,
                            EmbeddingLayer, SENETLayer)


class DeepFM(torch.nn.Module):
    def __init__(self, deep_features, fm_features, mlp_params):
        super(DeepFM, self).__init__()
        self.deep_features = deep_features
        self.fm_features = fm_features
        self.deep_dims = sum([fea.embed_dim for fea in deep_features])
        self.fm_dims = sum([fea.embed_dim for fea in fm_features])
        self.linear = LR(self.fm_dims)          # first order: ONE Linear over the flattened embeddings
        self.fm = FM(reduce_sum=True)           # second order
        self.embedding = EmbeddingLayer(deep_features + fm_features)
        self.mlp = MLP(self.deep_dims, **mlp_params)

    def _shared_gather(self):
        """True when the deep input is [the FM embeddings flattened | dense values]: the sparse features of
        ``deep_features`` are exactly ``fm_features`` in the same order (how deepfm.py is used with Criteo)."""
        sparse = [f for f in self.deep_features if not isinstance(f, DenseFeature)]
        return (len(sparse) == len(self.fm_features) and all(a is b for a, b in zip(sparse, self.fm_features))
                and len(set(f.embed_dim for f in self.fm_features)) == 1
                and all(isinstance(f, SparseFeature) for f in self.fm_features))

    def forward(self, x):
        if self._shared_gather():
            # deepfm.py:34-35 looks every table up twice (deep input, FM input) and autograd then adds two dense
            # [V, D] gradients per table.  Here ONE gather produces [B, F*D | dense] (rows padded to 16 bytes); the
            # FM part and the LR part read its leading F*D columns in place, the tower reads the whole row.
            input_deep = self.embedding(x, self.deep_features, squeeze_dim=True)
            dim = self.fm_features[0].embed_dim
            mods = self.mlp.mlp
            if (ops.config.fuse_deepfm_input and len(mods) > 0 and type(mods[0]) is torch.nn.Linear
                    and not self.linear.sigmoid and ops.deepfm_input_stage_supported(input_deep, self.fm_dims, dim)):
                # the three readers of the block as ONE autograd node: its gradient comes out of the tower's dx GEMM
                h, y_fm, y_linear = ops.deepfm_input_stage(input_deep, mods[0], self.linear.fc, self.fm_dims, dim)
                y_deep = dense.run_sequential(mods[1:], h)
                return ops.sigmoid_output((y_linear + y_fm + y_deep).squeeze(1))
            if input_deep.is_cuda and input_deep.dim() == 2:
                # three readers of one block: its gradient is assembled by one kernel (ops.shared_prefix)
                input_deep, flat_fm, flat_lr = ops.shared_prefix(input_deep, self.fm_dims, copies=2)
            else:
                flat_fm = flat_lr = input_deep[:, :self.fm_dims]
            input_fm = flat_fm.view(flat_fm.shape[0], len(self.fm_features), self.fm_features[0].embed_dim)
            y_linear = self.linear(flat_lr)
        else:
            input_deep = self.embedding(x, self.deep_features, squeeze_dim=True)     # [B, deep_dims]
            input_fm = self.embedding(x, self.fm_features, squeeze_dim=False)        # [B, F, D]
            y_linear = self.linear(input_fm.flatten(start_dim=1))
        y_fm = self.fm(input_fm)
        y_deep = self.mlp(input_deep)
        y = y_linear + y_fm + y_deep
        return ops.sigmoid_output(y.squeeze(1))


class ActivationUnit(torch.nn.Module):
    """DIN's target attention over one behaviour sequence: ``attention`` (an MLP over [target, history, target - history,
    target * history], one score per position), optional softmax over the positions (no mask in rechub), weighted sum of
    the history.  history [B, L, E], target [B, E] -> [B, E]; both may be slices of wider blocks (read in place)."""

    def __init__(self, emb_dim, dims=None, activation="dice", use_softmax=False):
        super(ActivationUnit, self).__init__()
        self.emb_dim = emb_dim
        self.use_softmax = use_softmax
        self.attention = MLP(4 * emb_dim, dims=[36] if dims is None else dims, activation=activation)

    def forward(self, history, target):
        return dense.run_din_unit(self.attention.mlp, history, target, None, self.use_softmax)


class DIN(torch.nn.Module):
    """Deep Interest Network: every history feature is pooled by its own ActivationUnit against the target feature of the
    same position; [pooled histories | targets | profile features] feed a Dice MLP.  ``attention_mlp_params`` are the
    ActivationUnit's keyword arguments, ``mlp_params`` the final MLP's (its activation is always "dice")."""

    def __init__(self, features, history_features, target_features, mlp_params, attention_mlp_params):
        super(DIN, self).__init__()
        self.features = features
        self.history_features = history_features
        self.target_features = target_features
        self.num_history_features = len(history_features)
        self.all_dims = sum(f.embed_dim for f in features + history_features + target_features)
        self.embedding = EmbeddingLayer(features + history_features + target_features)
        self.attention_layers = torch.nn.ModuleList(ActivationUnit(f.embed_dim, **attention_mlp_params)
                                                    for f in history_features)
        self.mlp = MLP(self.all_dims, activation="dice", **mlp_params)

    def forward(self, x):
        profile = self.embedding(x, self.features)              # [B, n_features, E]
        history = self.embedding(x, self.history_features)      # [B, n_history, L, E]
        target = self.embedding(x, self.target_features)        # [B, n_target, E]
        pooled = [unit(history[:, i], target[:, i]) for i, unit in enumerate(self.attention_layers)]
        mlp_in = torch.cat(pooled + [target.flatten(start_dim=1), profile.flatten(start_dim=1)], dim=1)
        return torch.sigmoid(self.mlp(mlp_in).squeeze(1))


class FiBiNet(torch.nn.Module):
    """FiBiNET (fibinet.py): the bilinear interactions of the field embeddings and of their SENET-gated copies feed an MLP.
    ``num_fields`` counts the unshared ``SparseFeature``s, the embedding width is the largest ``embed_dim``, the MLP reads
    ``F (F - 1) D`` columns.  The forward is one lookup, one ``ops.senet_gate`` and one ``ops.bilinear_pairs(..., scale=a)``
    whose [B, 2 P, D] result is the MLP's input viewed flat: no gated copy of x, no second interaction, no concatenation."""

    def __init__(self, features, mlp_params, reduction_ratio=3, bilinear_type="field_interaction", **kwargs):
        super(FiBiNet, self).__init__()
        self.features = features
        self.embedding = EmbeddingLayer(features)
        embedding_dim = max([fea.embed_dim for fea in features])
        num_fields = len([fea.embed_dim for fea in features if isinstance(fea, SparseFeature) and fea.shared_with is None])
        self.senet_layer = SENETLayer(num_fields, reduction_ratio)
        self.bilinear_interaction = BiLinearInteractionLayer(embedding_dim, num_fields, bilinear_type)
        self.dims = num_fields * (num_fields - 1) * embedding_dim
        self.mlp = MLP(self.dims, **mlp_params)

    def forward(self, x):
        from .multi_task import _embed, _mlp                            # the lookup and the MLP for CPU tensors as well
        embed_x = _embed(self.embedding, x, self.features, False)       # [B, F, D]
        a = self.senet_layer.gate(embed_x)                              # [B, F]
        shallow_part = self.bilinear_interaction(embed_x, a)            # [B, 2 P, D]: rows of x, then rows of x * a
        mlp_out = _mlp(self.mlp, shallow_part.flatten(start_dim=1))
        return torch.sigmoid(mlp_out.squeeze(1))


class _DeepFFMBase(torch.nn.Module):
    """What DeepFFM and FatDeepFFM share (deepffm.py:27-66 / :83-123): a first-order part summed over ``linear_features``, the
    field-aware crosses of ``cross_features`` -- feature i owns a table of ``vocab_i * F`` rows, id x names rows
    x * F .. x * F + F - 1 -- an MLP over them, and a bias ``b``."""

    def _build(self, linear_features, cross_features, embed_dim, mlp_params):
        self.linear_features = linear_features
        self.cross_features = cross_features
        self.num_fields = len(cross_features)
        self.num_field_cross = self.num_fields * (self.num_fields - 1) // 2
        self.ffm = FFM(num_fields=self.num_fields, reduce_sum=False)
        self.mlp_out = MLP(self.num_field_cross * embed_dim, **mlp_params)
        self.linear_embedding = EmbeddingLayer(linear_features)
        self.ffm_embedding = EmbeddingLayer(cross_features)
        self.b = torch.nn.Parameter(torch.zeros(1))
        self.register_buffer('fields_offset', torch.arange(0, self.num_fields, dtype=torch.long))

    def _ffm_tables(self):
        return [self.ffm_embedding.embed_dict[f.name if f.shared_with is None else f.shared_with]
                for f in self.cross_features]

    def _ffm_padding(self):
        """One entry per cross feature: the padding_idx its feature or its table declares (None = unset).  The reference
        looks such a feature up like any other; the fused op's gate refuses it and the composition serves it."""
        return [f.padding_idx if f.padding_idx is not None else t.padding_idx
                for f, t in zip(self.cross_features, self._ffm_tables())]

    def _crosses(self, x):
        """[B, P, D]: ``ops.ffm_cross`` on the raw ids and the tables; what its gate refuses (a width that is no multiple
        of 4, F * D > 1024, a padding_idx, a shared table, ...) runs the reference's composition."""
        tables = self._ffm_tables()
        ids = [x[f.name] for f in self.cross_features]
        weights = [t.weight for t in tables]
        if ops.config.ffm_fused and ops.ffm_supported(weights, ids, self._ffm_padding()):
            return ops.ffm_cross(weights, [t.reshape(-1) for t in ids], reduce_sum=False)
        rows = [torch.nn.functional.embedding(i.long().reshape(-1, 1) * self.num_fields + self.fields_offset, t.weight,
                                              t.padding_idx) for i, t in zip(ids, tables)]
        return self.ffm(torch.stack(rows, dim=1))                 # [B, F, F, D] -> [B, P, D]

    def _linear(self, x):
        return self.linear_embedding(x, self.linear_features, squeeze_dim=True).sum(1, keepdim=True)


class DeepFFM(_DeepFFMBase):
    def __init__(self, linear_features, cross_features, embed_dim, mlp_params):
        super().__init__()
        self._build(linear_features, cross_features, embed_dim, mlp_params)

    def forward(self, x):
        y_linear = self._linear(x)
        em = self._crosses(x)
        y_ffm = self.mlp_out(em.flatten(start_dim=1))
        y = y_linear + y_ffm
        return torch.sigmoid(y.squeeze(1) + self.b)


class FatDeepFFM(_DeepFFMBase):
    def __init__(self, linear_features, cross_features, embed_dim, reduction_ratio, mlp_params):
        super().__init__()
        self._build(linear_features, cross_features, embed_dim, mlp_params)
        self.cen = CEN(embed_dim, self.num_field_cross, reduction_ratio)

    def forward(self, x):
        y_linear = self._linear(x)
        em = self._crosses(x)
        aem = self.cen(em)
        y_ffm = self.mlp_out(aem)
        y = y_linear + y_ffm
        return torch.sigmoid(y.squeeze(1) + self.b)


# ---- Deep & Cross family (dcn.py, dcn_v2.py, edcn.py, widedeep.py) ------------------------------------------------------------
def _seq(seq, x):
    """An ``nn.Sequential`` over the dense kernels on the GPU, as it stands for CPU tensors."""
    return dense.run_sequential(seq, x) if x.is_cuda else seq(x)


def _lr(lr, x):
    from .multi_task import _linear
    y = _linear(x, lr.fc)
    return torch.sigmoid(y) if lr.sigmoid else y


class WideDeep(torch.nn.Module):
    """Wide & Deep (widedeep.py): an LR over the flattened ``wide_features`` plus an MLP over the ``deep_features``."""

    def __init__(self, wide_features, deep_features, mlp_params):
        super(WideDeep, self).__init__()
        self.wide_features = wide_features
        self.deep_features = deep_features
        self.wide_dims = sum([fea.embed_dim for fea in wide_features])
        self.deep_dims = sum([fea.embed_dim for fea in deep_features])
        self.linear = LR(self.wide_dims)
        self.embedding = EmbeddingLayer(wide_features + deep_features)
        self.mlp = MLP(self.deep_dims, **mlp_params)

    def forward(self, x):
        from .multi_task import _embed, _mlp
        input_wide = _embed(self.embedding, x, self.wide_features, True)
        input_deep = _embed(self.embedding, x, self.deep_features, True)
        y = _lr(self.linear, input_wide) + _mlp(self.mlp, input_deep)
        return torch.sigmoid(y.squeeze(1))


class DCN(torch.nn.Module):
    """Deep & Cross Network (dcn.py): ``CrossNetwork`` and an MLP without output layer read the flattened embeddings side by
    side; an LR over [cross | mlp] gives the logit."""

    def __init__(self, features, n_cross_layers, mlp_params):
        super().__init__()
        self.features = features
        self.dims = sum([fea.embed_dim for fea in features])
        self.embedding = EmbeddingLayer(features)
        self.cn = CrossNetwork(self.dims, n_cross_layers)
        self.mlp = MLP(self.dims, output_layer=False, **mlp_params)
        self.linear = LR(self.dims + mlp_params["dims"][-1])

    def forward(self, x):
        from .multi_task import _embed, _mlp
        embed_x = _embed(self.embedding, x, self.features, True)
        x_stack = torch.cat([self.cn(embed_x), _mlp(self.mlp, embed_x)], dim=1)
        return torch.sigmoid(_lr(self.linear, x_stack).squeeze(1))


class DCNv2(torch.nn.Module):
    """DCN-V2 (dcn_v2.py): ``CrossNetMix`` (``use_low_rank_mixture``, the default: one ``ops.cross_mix`` call for the stack) or
    ``CrossNetV2``; ``model_structure`` 'parallel' (cross beside ``parallel_dnn``), 'stacked' (``stacked_dnn`` after the cross
    net) or 'crossnet_only'; an LR gives the logit."""

    def __init__(self, features, n_cross_layers, mlp_params, model_structure="parallel", use_low_rank_mixture=True, low_rank=32,
                 num_experts=4, **kwargs):
        super(DCNv2, self).__init__()
        self.features = features
        self.dims = sum([fea.embed_dim for fea in features])
        self.embedding = EmbeddingLayer(features)
        if use_low_rank_mixture:
            self.crossnet = CrossNetMix(self.dims, n_cross_layers, low_rank=low_rank, num_experts=num_experts)
        else:
            self.crossnet = CrossNetV2(self.dims, n_cross_layers)
        self.model_structure = model_structure
        assert self.model_structure in ["crossnet_only", "stacked", "parallel"], \
            "model_structure={} not supported!".format(self.model_structure)
        if self.model_structure == "stacked":
            self.stacked_dnn = MLP(self.dims, output_layer=False, **mlp_params)
            final_dim = mlp_params["dims"][-1]
        if self.model_structure == "parallel":
            self.parallel_dnn = MLP(self.dims, output_layer=False, **mlp_params)
            final_dim = mlp_params["dims"][-1] + self.dims
        if self.model_structure == "crossnet_only":
            final_dim = self.dims
        self.linear = LR(final_dim)

    def forward(self, x):
        from .multi_task import _embed, _mlp
        embed_x = _embed(self.embedding, x, self.features, True)
        cross_out = self.crossnet(embed_x)
        if self.model_structure == "crossnet_only":
            final_out = cross_out
        elif self.model_structure == "stacked":
            final_out = _mlp(self.stacked_dnn, cross_out)
        else:
            final_out = torch.cat([cross_out, _mlp(self.parallel_dnn, embed_x)], dim=1)
        return torch.sigmoid(_lr(self.linear, final_out).squeeze(1))


class BridgeModule(torch.nn.Module):
    """EDCN's bridge between the cross and the deep branch (edcn.py BridgeModule): 'hadamard_product', 'pointwise_addition',
    'concatenation' (``concat_pooling``: Linear(2 n, n), ReLU) or 'attention_pooling' (``attention_x`` / ``attention_h``:
    Linear, ReLU, bias-free Linear, Softmax)."""

    def __init__(self, input_dim, bridge_type):
        super(BridgeModule, self).__init__()
        assert bridge_type in ["hadamard_product", "pointwise_addition", "concatenation",
                               "attention_pooling"], 'bridge_type= is not supported'.format(bridge_type)
        self.bridge_type = bridge_type
        if bridge_type == "concatenation":
            self.concat_pooling = torch.nn.Sequential(torch.nn.Linear(input_dim * 2, input_dim), torch.nn.ReLU())
        elif bridge_type == "attention_pooling":
            self.attention_x = torch.nn.Sequential(torch.nn.Linear(input_dim, input_dim), torch.nn.ReLU(),
                                                   torch.nn.Linear(input_dim, input_dim, bias=False), torch.nn.Softmax(dim=-1))
            self.attention_h = torch.nn.Sequential(torch.nn.Linear(input_dim, input_dim), torch.nn.ReLU(),
                                                   torch.nn.Linear(input_dim, input_dim, bias=False), torch.nn.Softmax(dim=-1))

    def forward(self, x, h):
        if self.bridge_type == "hadamard_product":
            out = x * h
        elif self.bridge_type == "pointwise_addition":
            out = x + h
        elif self.bridge_type == "concatenation":
            out = _seq(self.concat_pooling, torch.cat([x, h], dim=-1))
        elif self.bridge_type == "attention_pooling":
            out = _seq(self.attention_x, x) * x + _seq(self.attention_h, h) * h
        return out


class RegulationModule(torch.nn.Module):
    """EDCN's field-wise gates (edcn.py RegulationModule), as written there: ``g1`` / ``g2`` [num_fields], each entry soft-maxed
    on its own (a softmax over one element: 1) and repeated over its field's columns."""

    def __init__(self, num_fields, dims, tau, use_regulation=True):
        super(RegulationModule, self).__init__()
        self.use_regulation = use_regulation
        if self.use_regulation:
            self.num_fields = num_fields
            self.dims = dims
            self.tau = tau
            self.g1 = torch.nn.Parameter(torch.ones(num_fields))
            self.g2 = torch.nn.Parameter(torch.ones(num_fields))

    def forward(self, x):
        if self.use_regulation:
            g1 = torch.cat([(self.g1[i] / self.tau).softmax(dim=-1).unsqueeze(-1).repeat(1, self.dims[i])
                            for i in range(self.num_fields)], dim=-1)
            g2 = torch.cat([(self.g2[i] / self.tau).softmax(dim=-1).unsqueeze(-1).repeat(1, self.dims[i])
                            for i in range(self.num_fields)], dim=-1)
            out1, out2 = g1 * x, g2 * x
        else:
            out1, out2 = x, x
        return out1, out2


class EDCN(torch.nn.Module):
    """Enhanced DCN (edcn.py): per layer a ``CrossLayer`` with its residual and an MLP of dims [n, n] run side by side, joined by
    a ``BridgeModule`` and split again by a ``RegulationModule``; an LR over [cross | deep | bridge].  As in the reference, the
    caller's ``mlp_params["dims"]`` is overwritten with [n, n]."""

    def __init__(self, features, n_cross_layers, mlp_params, bridge_type="hadamard_product", use_regulation_module=True,
                 temperature=1):
        super().__init__()
        self.features = features
        self.n_cross_layers = n_cross_layers
        self.num_fields = len(features)
        self.dims = sum([fea.embed_dim for fea in features])
        self.fea_dims = [fea.embed_dim for fea in features]
        self.embedding = EmbeddingLayer(features)
        self.cross_layers = torch.nn.ModuleList([CrossLayer(self.dims) for _ in range(n_cross_layers)])
        self.bridge_modules = torch.nn.ModuleList([BridgeModule(self.dims, bridge_type) for _ in range(n_cross_layers)])
        self.regulation_modules = torch.nn.ModuleList([RegulationModule(self.num_fields, self.fea_dims, tau=temperature,
                                                                        use_regulation=use_regulation_module)
                                                       for _ in range(n_cross_layers)])
        mlp_params["dims"] = [self.dims, self.dims]
        self.mlps = torch.nn.ModuleList([MLP(self.dims, output_layer=False, **mlp_params) for _ in range(n_cross_layers)])
        self.linear = LR(self.dims * 3)

    def forward(self, x):
        from .multi_task import _embed, _mlp
        embed_x = _embed(self.embedding, x, self.features, True)
        cross_i, deep_i = self.regulation_modules[0](embed_x)
        cross_0 = cross_i
        for i in range(self.n_cross_layers):
            if i > 0:
                cross_i, deep_i = self.regulation_modules[i](bridge_i)
            cross_i = self.cross_layers[i].residual(cross_0, cross_i)
            deep_i = _mlp(self.mlps[i], deep_i)
            bridge_i = self.bridge_modules[i](cross_i, deep_i)
        x_stack = torch.cat([cross_i, deep_i, bridge_i], dim=1)
        return torch.sigmoid(_lr(self.linear, x_stack).squeeze(1))


# ---- Attentional FM (RecBole's AFM in the rechub style) -----------------------------------------------------------------------
class AFM(torch.nn.Module):
    """Attentional FM as a trainable model in the style of this zoo: ``EmbeddingLayer`` over ``features`` (unshared
    ``SparseFeature``s of one ``embed_dim``), an ``LR`` over the flattened embeddings as the first-order term, and
    ``recbole.context_aware.AFMInteraction`` (one ``ops.afm_pool`` launch each way) as the second-order term; the output is
    ``sigmoid(first + second)`` [B].  ``interaction.state_dict()`` has RecBole's AFM keys (``attlayer.w.weight``, ``attlayer.h``,
    ``p``).  RecBole's ``AFM(config, dataset)`` constructor, its ``ContextRecommender`` base (field-typed embedding tables and
    ``first_order_linear``) and ``calculate_loss`` are NOT mirrored: add ``interaction.reg_loss(reg_weight)`` to the loss for
    the reference's L2 term."""

    def __init__(self, features, attention_size=25, dropout_prob=0.3):
        super(AFM, self).__init__()
        from ...recbole.context_aware import AFMInteraction
        dims = set(fea.embed_dim for fea in features)
        if len(dims) != 1 or len(features) < 2:
            raise ValueError("AFM: at least two features of one embed_dim (got dims %s)" % sorted(dims))
        self.features = features
        self.embedding = EmbeddingLayer(features)
        self.num_fields = len(features)
        self.embed_dim = dims.pop()
        self.linear = LR(self.num_fields * self.embed_dim)
        self.interaction = AFMInteraction(self.num_fields, self.embed_dim, attention_size, dropout_prob)

    def forward(self, x):
        from .multi_task import _embed
        embed_x = _embed(self.embedding, x, self.features, False)          # [B, F, D]
        y = _lr(self.linear, embed_x.flatten(start_dim=1)) + self.interaction(embed_x)
        return torch.sigmoid(y.squeeze(1))


# ---- Deep Interest Evolution Network (RecBole's DIEN in the rechub style) -------------------------------------------------------
class DIEN(torch.nn.Module):
    """DIEN as a trainable model in the style of this zoo, beside ``DIN``: ``EmbeddingLayer`` over ``features`` (profile),
    ``history_features`` and ``neg_history_features`` (``SequenceFeature``s with ``pooling="concat"``, usually
    ``shared_with`` the target's table; the negatives are the sampled non-clicked behaviours of the auxiliary loss) and
    ``target_features``.  The history embeddings are concatenated over the history features into [B, L, E] and the targets
    into [B, E] (so the widths must agree); the lengths are counted on the device from the first history feature's non-zero
    ids (left-aligned histories, at least one behaviour per sample).  ``recbole.sequential.InterestExtractorNetwork`` (``ops.gru``)
    and ``InterestEvolvingLayer`` (``gru_type`` in 'GRU', 'AIGRU', 'AGRU', 'AUGRU'; the last two on ``ops.att_gru``) give the
    evolved interest; [evolution | targets | profile features] feed a Dice MLP as in ``DIN``.  ``attention_mlp_params``:
    ``dims`` (the hidden sizes of the score MLP, default [80, 40]) and ``activation`` (default "sigmoid"); the auxiliary net
    has ``mlp_params["dims"]`` hidden sizes.  ``forward(x)`` returns ``(sigmoid prediction [B], aux_loss)``; the training loss
    is ``bce + model.alpha * aux_loss``.  RecBole's ``DIEN(config, dataset)`` constructor, ``ContextSeqEmbLayer`` and
    ``calculate_loss`` are NOT mirrored."""

    def __init__(self, features, history_features, neg_history_features, target_features, mlp_params, attention_mlp_params,
                 gru_type="AUGRU", alpha=1.0):
        super(DIEN, self).__init__()
        from ...recbole.sequential import InterestEvolvingLayer, InterestExtractorNetwork
        if gru_type not in ("GRU", "AIGRU", "AGRU", "AUGRU"):
            raise ValueError("DIEN: gru_type must be GRU, AIGRU, AGRU or AUGRU (got %r)" % (gru_type,))
        self.features = features
        self.history_features = history_features
        self.neg_history_features = neg_history_features
        self.target_features = target_features
        self.gru_type = gru_type
        self.alpha = alpha
        self.item_dim = sum(f.embed_dim for f in history_features)
        if (not history_features or len(neg_history_features) != len(history_features)
                or sum(f.embed_dim for f in target_features) != self.item_dim
                or sum(f.embed_dim for f in neg_history_features) != self.item_dim):
            raise ValueError("DIEN: history, negative history and target features must have the same total width")
        self.embedding = EmbeddingLayer(features + history_features + neg_history_features + target_features)
        att = dict(attention_mlp_params or {})
        att_dims = [4 * self.item_dim] + list(att.get("dims", [80, 40]))
        self.interest_extractor = InterestExtractorNetwork(self.item_dim, self.item_dim,
                                                           [2 * self.item_dim] + list(mlp_params["dims"]) + [1])
        self.interest_evolution = InterestEvolvingLayer(None, self.item_dim, self.item_dim, att_dims,
                                                        activation=att.get("activation", "sigmoid"), gru=gru_type)
        self.all_dims = 2 * self.item_dim + sum(f.embed_dim for f in features)
        self.mlp = MLP(self.all_dims, activation="dice", **mlp_params)

    def _sequence(self, x, features):
        from .multi_task import _embed
        rows = _embed(self.embedding, x, features, False)                   # [B, n, L, E_f]
        B, n, L, E = rows.shape
        return rows.permute(0, 2, 1, 3).reshape(B, L, n * E)

    def forward(self, x):
        from .multi_task import _embed, _mlp
        history = self._sequence(x, self.history_features)                  # [B, L, E]
        negatives = self._sequence(x, self.neg_history_features)
        target = _embed(self.embedding, x, self.target_features, False).flatten(start_dim=1)         # [B, E]
        lengths = (x[self.history_features[0].name] != 0).sum(dim=1)
        interest, aux_loss = self.interest_extractor(history, lengths, negatives)
        evolution = self.interest_evolution(target, interest, lengths)
        parts = [evolution, target]
        if self.features:
            parts.append(_embed(self.embedding, x, self.features, False).flatten(start_dim=1))
        return torch.sigmoid(_mlp(self.mlp, torch.cat(parts, dim=1)).squeeze(1)), aux_loss


# ---- AutoInt (RecBole's AutoInt in the rechub style) --------------------------------------------------------------------------
class AutoInt(torch.nn.Module):
    """AutoInt as a trainable model in the style of this zoo: ``EmbeddingLayer`` over ``features`` (unshared ``SparseFeature``s
    of one ``embed_dim``), an ``LR`` over the flattened embeddings as the first-order term, and
    ``recbole.context_aware.AutoIntInteraction`` (one ``ops.field_attn`` launch each way per layer) for the attention and MLP
    terms; the output is ``sigmoid(first + interaction)`` [B].  ``interaction.state_dict()`` has RecBole's AutoInt keys.
    RecBole's ``AutoInt(config, dataset)`` constructor, its ``ContextRecommender`` base and ``calculate_loss`` are NOT
    mirrored."""

    def __init__(self, features, attention_size=16, n_layers=3, num_heads=2, mlp_hidden_size=(128, 128),
                 dropout_probs=(0.2, 0.2, 0.2), has_residual=True):
        super(AutoInt, self).__init__()
        from ...recbole.context_aware import AutoIntInteraction
        dims = set(fea.embed_dim for fea in features)
        if len(dims) != 1 or len(features) < 2:
            raise ValueError("AutoInt: at least two features of one embed_dim (got dims %s)" % sorted(dims))
        self.features = features
        self.embedding = EmbeddingLayer(features)
        self.num_fields = len(features)
        self.embed_dim = dims.pop()
        self.linear = LR(self.num_fields * self.embed_dim)
        self.interaction = AutoIntInteraction(self.num_fields, self.embed_dim, attention_size, n_layers, num_heads,
                                              list(mlp_hidden_size), list(dropout_probs), has_residual)

    def forward(self, x):
        from .multi_task import _embed
        embed_x = _embed(self.embedding, x, self.features, False)          # [B, F, D]
        y = _lr(self.linear, embed_x.flatten(start_dim=1)) + self.interaction(embed_x)
        return torch.sigmoid(y.squeeze(1))


# ---- FiGNN (RecBole's FiGNN in the rechub style) ------------------------------------------------------------------------------
class FiGNN(torch.nn.Module):
    """FiGNN as a trainable model in the style of this zoo: ``EmbeddingLayer`` over ``features`` (unshared ``SparseFeature``s of
    one ``embed_dim``) and ``recbole.context_aware.FiGNNInteraction`` (one ``ops.field_attn`` launch, then one
    ``ops.fignn_step`` launch each way per message-passing layer, then the attentional scoring); the output is
    ``sigmoid(fignn_layer(embeddings))`` [B], as the reference's ``predict``.  ``interaction.state_dict()`` has RecBole's FiGNN
    keys.  RecBole's ``FiGNN(config, dataset)`` constructor, its ``ContextRecommender`` base and ``calculate_loss`` are NOT
    mirrored."""

    def __init__(self, features, attention_size=16, n_layers=3, num_heads=2, hidden_dropout=0.2, attn_dropout=0.2):
        super(FiGNN, self).__init__()
        from ...recbole.context_aware import FiGNNInteraction
        dims = set(fea.embed_dim for fea in features)
        if len(dims) != 1 or len(features) < 2:
            raise ValueError("FiGNN: at least two features of one embed_dim (got dims %s)" % sorted(dims))
        self.features = features
        self.embedding = EmbeddingLayer(features)
        self.num_fields = len(features)
        self.embed_dim = dims.pop()
        self.interaction = FiGNNInteraction(self.num_fields, self.embed_dim, attention_size, n_layers, num_heads, hidden_dropout,
                                            attn_dropout)

    def forward(self, x):
        from .multi_task import _embed
        embed_x = _embed(self.embedding, x, self.features, False)          # [B, F, D]
        return torch.sigmoid(self.interaction(embed_x).squeeze(1))
