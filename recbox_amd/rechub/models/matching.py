"""Two-tower and sequential matching models (drop-in for ``torch_rechub.models.matching.
{DSSM, YoutubeDNN, SASRec}``, /root/reference/recbox/third_party/rechub/models/matching/
dssm.py:15-66, youtube_dnn.py:14-71, sasrec.py:17-124): same constructors, ``mode`` switch,
outputs and parameter names.  Compute: embedding + pooling in one gather launch, MLP Linear
layers on the fp32 matrix cores, ``F.normalize`` and the pairwise dot as HIP kernels
(``rbx_l2norm_*``, ``rbx_pairdot_*``), SASRec's causal attention as the fused LDS-resident
kernel (``rbx_attn_*``)."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import ops
from ..basic.features import DenseFeature, SequenceFeature, SparseFeature
from ..basic.layers import GRU, MLP, CapsuleNetwork, EmbeddingLayer, MultiInterestSA
# a lookup / a tower of YoutubeSBC and FaceBookDSSM: the shared layers on the GPU, the reference's lines in ATen for CPU tensors
from .multi_task import _embed as _embed_any, _mlp


class DSSM(torch.nn.Module):
    def __init__(self, user_features, item_features, user_params, item_params, temperature=1.0):
        super().__init__()
        self.user_features = user_features
        self.item_features = item_features
        self.temperature = temperature
        self.user_dims = sum([fea.embed_dim for fea in user_features])
        self.item_dims = sum([fea.embed_dim for fea in item_features])
        self.embedding = EmbeddingLayer(user_features + item_features)
        self.user_mlp = MLP(self.user_dims, output_layer=False, **user_params)
        self.item_mlp = MLP(self.item_dims, output_layer=False, **item_params)
        self.mode = None

    def forward(self, x):
        user_embedding = self.user_tower(x)
        item_embedding = self.item_tower(x)
        if self.mode == "user":
            return user_embedding
        if self.mode == "item":
            return item_embedding
        y = ops.pair_dot(user_embedding, item_embedding).squeeze(1)      # cosine score [B]
        return torch.sigmoid(y)                                          # (the reference leaves /temperature out)

    def user_tower(self, x):
        if self.mode == "item":
            return None
        input_user = self.embedding(x, self.user_features, squeeze_dim=True)
        return ops.l2_normalize(self.user_mlp(input_user))

    def item_tower(self, x):
        if self.mode == "user":
            return None
        input_item = self.embedding(x, self.item_features, squeeze_dim=True)
        return ops.l2_normalize(self.item_mlp(input_item))


class YoutubeDNN(torch.nn.Module):
    def __init__(self, user_features, item_features, neg_item_feature, user_params, temperature=1.0):
        super().__init__()
        self.user_features = user_features
        self.item_features = item_features
        self.neg_item_feature = neg_item_feature
        self.temperature = temperature
        self.user_dims = sum([fea.embed_dim for fea in user_features])
        self.embedding = EmbeddingLayer(user_features + item_features)
        self.user_mlp = MLP(self.user_dims, output_layer=False, **user_params)
        self.mode = None

    def forward(self, x):
        if self.mode is None and not any(isinstance(f, DenseFeature) for f in self.user_features):
            # training: ONE gather launch (and one backward scatter-add) for the user side, the positive item and
            # the negatives.  The history, the positive and the negatives share one table; looking them up in two
            # calls, as youtube_dnn.py:52-70 does, would build two dense [V, D] gradients of that table and add them.
            dim = self.item_features[0].embed_dim
            both = self.embedding(x, self.user_features + self.item_features + self.neg_item_feature, squeeze_dim=True)
            # the two column blocks in place (the tower's first GEMM and the normalisation take a row stride); backward = one
            # concatenation
            user_in, items = ops.split_last(both, self.user_dims, views=True)
            user_embedding = ops.l2_normalize(self.user_mlp(user_in))
            # F.normalize of the item rows + the inner product in one pass over them (rbx_cosdot_*): the normalised
            # [B, 1 + n_neg, D] block is never written, and its gradient lands in a block of `both`'s shape
            return ops.cos_dot(user_embedding, items.unflatten(1, (-1, dim)), eps=1e-12,
                               scale=1.0 / self.temperature)                                    # [B, 1 + n_neg]
        # (a squeezed gather lays DenseFeature values out AFTER every embedding of the call -- layers.py:109-114 --, so
        #  with dense user features the single gather above would put them behind the item / negative rows: the towers
        #  are then looked up separately, as youtube_dnn.py:46-70 does)
        user_embedding = self.user_tower(x)
        item_embedding = self.item_tower(x)
        if self.mode == "user":
            return user_embedding
        if self.mode == "item":
            return item_embedding
        return ops.pair_dot(user_embedding, item_embedding, scale=1.0 / self.temperature)       # [B, 1 + n_neg]

    def user_tower(self, x):
        if self.mode == "item":
            return None
        input_user = self.embedding(x, self.user_features, squeeze_dim=True)
        user_embedding = ops.l2_normalize(self.user_mlp(input_user)).unsqueeze(1)           # [B, 1, D]
        if self.mode == "user":
            return user_embedding.squeeze(1)
        return user_embedding

    def item_tower(self, x):
        if self.mode == "user":
            return None
        if self.mode == "item":
            pos = self.embedding(x, self.item_features, squeeze_dim=False)                  # [B, 1, D]
            return ops.l2_normalize(pos).squeeze(1)
        # positive id and the n_neg negative ids in ONE gather launch: [B, (1 + n_neg) * D]
        both = self.embedding(x, self.item_features + self.neg_item_feature, squeeze_dim=True)
        dim = self.item_features[0].embed_dim
        return ops.l2_normalize(both.reshape(both.shape[0], -1, dim))                          # [B, 1 + n_neg, D]


class PointWiseFeedForward(torch.nn.Module):
    def __init__(self, hidden_units, dropout_rate):
        super(PointWiseFeedForward, self).__init__()
        self.conv1 = torch.nn.Conv1d(hidden_units, hidden_units, kernel_size=1)
        self.dropout1 = torch.nn.Dropout(p=dropout_rate)
        self.relu = torch.nn.ReLU()
        self.conv2 = torch.nn.Conv1d(hidden_units, hidden_units, kernel_size=1)
        self.dropout2 = torch.nn.Dropout(p=dropout_rate)

    def branch(self, inputs):
        """The two 1x1 convolutions without the residual connection."""
        # a kernel-size-1 Conv1d over [B, C, L] is a Linear over the channel axis of [B, L, C]
        if self.dropout1.p > 0 and self.training:
            h = self.relu(self.dropout1(ops.linear(inputs, self.conv1.weight.squeeze(-1), self.conv1.bias)))
        else:
            h = ops.linear(inputs, self.conv1.weight.squeeze(-1), self.conv1.bias, act="relu")
        return self.dropout2(ops.linear(h, self.conv2.weight.squeeze(-1), self.conv2.bias))

    def forward(self, inputs):
        return self.branch(inputs) + inputs


class SASRec(torch.nn.Module):
    """features = [seq, pos, neg] SequenceFeatures (pooling='concat', pos/neg shared_with seq)."""

    def __init__(self, features, max_len=50, dropout_rate=0.5, num_blocks=2, num_heads=1):
        super(SASRec, self).__init__()
        self.features = features
        self.item_num = self.features[0].vocab_size
        self.embed_dim = self.features[0].embed_dim
        self.item_emb = EmbeddingLayer(self.features)
        self.position_emb = torch.nn.Embedding(max_len, self.embed_dim)
        self.emb_dropout = torch.nn.Dropout(p=dropout_rate)
        self.attention_layernorms = torch.nn.ModuleList()
        self.attention_layers = torch.nn.ModuleList()
        self.forward_layernorms = torch.nn.ModuleList()
        self.forward_layers = torch.nn.ModuleList()
        self.last_layernorm = torch.nn.LayerNorm(self.embed_dim, eps=1e-8)
        for _ in range(num_blocks):
            self.attention_layernorms.append(torch.nn.LayerNorm(self.embed_dim, eps=1e-8))
            self.attention_layers.append(torch.nn.MultiheadAttention(self.embed_dim, num_heads, dropout_rate))
            self.forward_layernorms.append(torch.nn.LayerNorm(self.embed_dim, eps=1e-8))
            self.forward_layers.append(PointWiseFeedForward(self.embed_dim, dropout_rate))

    def _mha(self, layer, query, keyval):
        """nn.MultiheadAttention(query, keyval, keyval, attn_mask=causal) on [B, L, E] tensors."""
        p_drop = layer.dropout if self.training else 0.0      # dropout on the probabilities, inside the fused kernel
        E, H = layer.embed_dim, layer.num_heads
        hd = E // H
        w, b = layer.in_proj_weight, layer.in_proj_bias
        q = ops.linear(query, w[:E], b[:E] if b is not None else None)
        kv = ops.linear(keyval, w[E:], b[E:] if b is not None else None)          # one GEMM for K and V
        B, L = query.shape[0], query.shape[1]
        if ops.attention_packed_supported(L, hd):
            # the kernels read Q [B, L, E] and K | V [B, L, 2 E] where the projections left them and write O [B, L, E],
            # dQ and dK | dV in place: no head transposes, no K / V split copies, no concatenation in the backward
            o = ops.attention_packed(q, kv, H, hd ** -0.5, causal=True, dropout_p=p_drop)
            return ops.linear(o, layer.out_proj.weight, layer.out_proj.bias)
        q = q.view(B, L, H, hd).transpose(1, 2)
        k, v = ops.split_last(kv, E)                            # contiguous halves; backward = one concatenation
        k = k.view(B, L, H, hd).transpose(1, 2)
        v = v.view(B, L, H, hd).transpose(1, 2)
        o, _ = ops.attention(q, k, v, mask=None, scale=hd ** -0.5, causal=True, fill=float("-inf"), dropout_p=p_drop)
        o = o.transpose(1, 2).reshape(B, L, E)
        return ops.linear(o, layer.out_proj.weight, layer.out_proj.bias)

    def seq_forward(self, x, embed_x_feature):
        ids = x['seq']
        e = embed_x_feature
        if e.dim() == 4:
            e = e.squeeze(1)
        positions = torch.arange(ids.shape[1], device=ids.device).unsqueeze(0).expand(ids.shape[0], -1)
        keep = (ids != 0).to(e.dtype)                         # ~timeline_mask, one value per (sample, position)
        scale = self.features[0].embed_dim ** 0.5
        input_stage = None
        if isinstance(self.emb_dropout, torch.nn.Dropout) and self.emb_dropout.p > 0 and self.training:
            e = self.emb_dropout(e * scale + ops_position(self.position_emb, positions))
            e = ops.row_scale(e, keep)
        elif (ops.config.seq_positions_in_place and e.dim() == 3 and self.position_emb.padding_idx is None
              and self.position_emb.max_norm is None and ids.shape[1] <= self.position_emb.num_embeddings):
            # positions are arange(L) for every sequence: the table's first L rows read in place, their gradient a column sum
            first = self.attention_layers[0] if len(self.attention_layers) else None
            ffn0 = self.forward_layers[0] if len(self.forward_layers) else None
            if (first is not None and ops.config.fuse_sublayers and ops.config.seqblock_bwd
                    and not (self.training and (ffn0.dropout1.p > 0 or ffn0.dropout2.p > 0))
                    and ops.seqblock_supported(e, first, False)):
                # ... and the stage itself belongs to the first block's node: its backward (de * keep * sqrt(D)) rides in
                # the store of the block's last backward pass instead of a pass of its own over [B L, D]
                input_stage = (self.position_emb.weight[:ids.shape[1]], scale)
            else:
                e = ops.sasrec_input(e, self.position_emb.weight[:ids.shape[1]], keep, alpha=scale)
        else:      # (e * sqrt(D) + position) * ~mask in one pass (rbx_rowscale) instead of three element-wise kernels
            e = ops.row_scale(e, keep, add=ops_position(self.position_emb, positions), alpha=scale)
        for i in range(len(self.attention_layers)):
            mha, ffn = self.attention_layers[i], self.forward_layers[i]
            stage, input_stage = input_stage, None
            E, H = mha.embed_dim, mha.num_heads
            ffn_drop = self.training and (ffn.dropout1.p > 0 or ffn.dropout2.p > 0)
            if ops.config.fuse_sublayers and ops.seqblock_supported(e, mha, ffn_drop):
                # the whole block as one autograd node: LayerNorm + in-projections, attention, out-projection + residual +
                # LayerNorm + FFN + residual + mask -- three launches forward (csrc/rbx_seqblock.hip)
                e = ops.sasrec_block(e, self.attention_layernorms[i], mha, self.forward_layernorms[i],
                                     ffn.conv1.weight.squeeze(-1), ffn.conv1.bias, ffn.conv2.weight.squeeze(-1), ffn.conv2.bias,
                                     keep, dropout_p=mha.dropout if self.training else 0.0, input_stage=stage)
                continue
            if (ops.config.fuse_sublayers and e.dim() == 3 and mha.in_proj_weight is not None
                    and ops.attention_packed_supported(e.shape[1], E // H)):
                # LayerNorm, the three projections, the attention and the residual as ONE autograd node: the residual add
                # and the two gradient sums of the backward live in GEMM epilogues
                e = ops.sasrec_attention_sublayer(e, self.attention_layernorms[i], mha,
                                                  dropout_p=mha.dropout if self.training else 0.0)
            else:
                q = ops.layer_norm(e, self.attention_layernorms[i])
                e = q + self._mha(mha, q, e)
            if ops.config.fuse_sublayers and e.dim() == 3 and not (self.training and (ffn.dropout1.p > 0 or ffn.dropout2.p > 0)):
                e = ops.sasrec_ffn_sublayer(e, self.forward_layernorms[i], ffn.conv1.weight.squeeze(-1), ffn.conv1.bias,
                                            ffn.conv2.weight.squeeze(-1), ffn.conv2.bias, keep, keep_is_mask=True)
            else:
                e = ops.layer_norm(e, self.forward_layernorms[i])
                # (ffn(e) + e) * ~mask: the residual add and the timeline mask in one pass
                e = ops.row_scale(ffn.branch(e), keep, add=e)
        return ops.layer_norm(e, self.last_layernorm)

    def forward(self, x):
        """sasrec.py:96-107.  The reference embeds seq, pos and neg ([B, 3, L, D]) and multiplies; here only the
        input sequence is materialised: the pos / neg logits come from rbx_gatherdot (K7), which reads each
        candidate row once and never writes the two [B, L, D] candidate tensors (nor their gradients)."""
        seq_f, cand_f = self.features[0], self.features[1:]
        seq_embed = self.item_emb(x, [seq_f])                 # [B, 1, L, D]
        # (a view, not seq_embed[:, 0]: the backward of a select is a zero fill + a copy of the whole [B, L, D] gradient --
        #  117 us per step at cfg 5, profiles/r04/INDEX.md; a view's backward is a view)
        seq_output = self.seq_forward(x, seq_embed.view(seq_embed.shape[0], seq_embed.shape[2], seq_embed.shape[3])
                                      if seq_embed.dim() == 4 and seq_embed.shape[1] == 1 else seq_embed[:, 0])
        B, L, D = seq_output.shape
        tables = [self.item_emb.embed_dict[f.name if f.shared_with is None else f.shared_with].weight for f in cand_f]
        logits = ops.gather_dot(seq_output.reshape(B * L, D), [x[f.name].reshape(-1) for f in cand_f], tables)
        return tuple(logits[:, c].reshape(B, L) for c in range(len(cand_f)))


def ops_position(position_emb, positions):
    """position_emb(positions) through the gather kernel (one-table lookup with a [B, L] id block)."""
    from ... import _embed_host as host
    from ..._lib import FIELD_CATEGORICAL, POOL_CONCAT
    plan = getattr(position_emb, "_rbx_plan", None)
    L = positions.shape[1]
    if plan is None or plan.specs[0].seq_len != L:
        plan = host.Plan([host.Lookup("position", FIELD_CATEGORICAL, position_emb, position_emb.embedding_dim,
                                      pool=POOL_CONCAT, seq_len=L)])
        position_emb._rbx_plan = plan
    out = plan.run([positions])
    return out.view(positions.shape[0], L, position_emb.embedding_dim)


class _MultiInterest(torch.nn.Module):
    """What MIND, ComirecDR and ComirecSA share (mind.py:32-101, comirec.py:17-188): an extractor over the history gives
    ``interest_num`` vectors per user; training scores the interest that fits the positive item best.  A subclass registers its
    extractor (after ``embedding``, as the reference does) and answers ``extract``."""

    def __init__(self, user_features, history_features, item_features, neg_item_feature, temperature=1.0, interest_num=4):
        super().__init__()
        self.user_features = user_features
        self.item_features = item_features
        self.history_features = history_features
        self.neg_item_feature = neg_item_feature
        self.temperature = temperature
        self.interest_num = interest_num
        self.user_dims = sum([fea.embed_dim for fea in user_features + history_features])
        self.embedding = EmbeddingLayer(user_features + item_features + history_features)
        self.convert_user_weight = nn.Parameter(torch.rand(self.user_dims, self.history_features[0].embed_dim),
                                                requires_grad=True)
        self.mode = None

    def extract(self, history_emb, x):
        """[B, L, D] -> [B, interest_num, D]"""
        raise NotImplementedError

    # the three places where a tower touches the kernels; ComirecSA, which also serves CPU tensors, overrides them
    def _embed(self, x, features, squeeze_dim=False):
        return self.embedding(x, features, squeeze_dim=squeeze_dim)

    def _project(self, input_user):
        return ops.linear(input_user, self.convert_user_weight.t())

    def _normalize(self, t):
        return ops.l2_normalize(t)

    def forward(self, x):
        user_embedding = self.user_tower(x)
        item_embedding = self.item_tower(x)
        if self.mode == "user":
            return user_embedding
        if self.mode == "item":
            return item_embedding
        # the interest with the largest inner product with the positive item: one argmax + gather instead of the reference's
        # Python loop over the batch (mind.py:57-62)
        pos = item_embedding[:, 0, :]
        k_index = torch.argmax(torch.bmm(user_embedding.detach(), pos.detach().unsqueeze(-1)), dim=1)      # [B, 1]
        best = torch.gather(user_embedding, 1, k_index.unsqueeze(-1).expand(-1, 1, user_embedding.shape[2]))
        return torch.mul(best, item_embedding).sum(dim=1)                                                  # [B, D], as written

    def user_tower(self, x):
        if self.mode == "item":
            return None
        input_user = self._embed(x, self.user_features, squeeze_dim=True).unsqueeze(1)
        input_user = input_user.expand([input_user.shape[0], self.interest_num, input_user.shape[-1]])
        history_emb = self._embed(x, self.history_features).squeeze(1)                                     # [B, L, D]
        multi_interest_emb = self.extract(history_emb, x)                                                  # [B, K, D]
        input_user = torch.cat([input_user, multi_interest_emb], dim=-1)
        return self._normalize(self._project(input_user))                                                  # [B, K, D]

    def item_tower(self, x):
        if self.mode == "user":
            return None
        pos_embedding = self._normalize(self._embed(x, self.item_features, squeeze_dim=False))             # [B, 1, D]
        if self.mode == "item":
            return pos_embedding.squeeze(1)
        neg_embeddings = self._normalize(self._embed(x, self.neg_item_feature, squeeze_dim=False).squeeze(1))
        return torch.cat((pos_embedding, neg_embeddings), dim=1)                                           # [B, 1 + n_neg, D]

    def gen_mask(self, x):
        his_list = x[self.history_features[0].name]
        return (his_list > 0).long()


class _MultiInterestDR(_MultiInterest):
    """The capsule-routing members (mind.py:32-101, comirec.py:118-188)."""
    bilinear_type = 2

    def __init__(self, user_features, history_features, item_features, neg_item_feature, max_length, temperature=1.0,
                 interest_num=4):
        super().__init__(user_features, history_features, item_features, neg_item_feature, temperature, interest_num)
        self.max_length = max_length
        self.capsule = CapsuleNetwork(self.history_features[0].embed_dim, self.max_length, bilinear_type=self.bilinear_type,
                                      interest_num=self.interest_num)

    def extract(self, history_emb, x):
        return self.capsule(history_emb, self.gen_mask(x))


class MIND(_MultiInterestDR):
    """``torch_rechub.models.matching.MIND`` (mind.py:17-101): ``CapsuleNetwork(bilinear_type=0)``, whose starting logits are
    drawn with one ``torch.randn`` per forward."""
    bilinear_type = 0


class ComirecDR(_MultiInterestDR):
    """``torch_rechub.models.matching.ComirecDR`` (comirec.py:103-188): ``CapsuleNetwork(bilinear_type=2)``."""
    bilinear_type = 2


def _embed_aten(layer, x, features, squeeze_dim):
    """``EmbeddingLayer.forward`` for CPU tensors, in ATen: one-hot features and ``pooling='concat'`` sequences, which is
    what the multi-interest models feed it."""
    rows = []
    for fea in features:
        table = layer.embed_dict[fea.name if fea.shared_with is None else fea.shared_with]
        if isinstance(fea, SparseFeature):
            rows.append(table(x[fea.name].long()).unsqueeze(1))                                            # [B, 1, D]
        elif isinstance(fea, SequenceFeature) and fea.pooling == "concat":
            rows.append(table(x[fea.name].long()).unsqueeze(1))                                            # [B, 1, L, D]
        else:
            raise NotImplementedError("feature '%s': the CPU path serves one-hot and pooling='concat' features" % fea.name)
    out = torch.cat(rows, dim=1)
    return out.flatten(start_dim=1) if squeeze_dim else out


class ComirecSA(_MultiInterest):
    """``torch_rechub.models.matching.ComirecSA`` (comirec.py:17-101): the towers of ComirecDR around ``MultiInterestSA``
    (``multi_interest_sa.W1`` / ``W2`` / ``W3``), which is one ``ops.sa_pool`` call.  No ``max_length``, as in the
    reference.  CPU tensors run the same model in ATen."""

    def __init__(self, user_features, history_features, item_features, neg_item_feature, temperature=1.0, interest_num=4):
        super().__init__(user_features, history_features, item_features, neg_item_feature, temperature, interest_num)
        self.multi_interest_sa = MultiInterestSA(embedding_dim=self.history_features[0].embed_dim, interest_num=self.interest_num)

    def extract(self, history_emb, x):
        return self.multi_interest_sa(history_emb, self.gen_mask(x))

    def _embed(self, x, features, squeeze_dim=False):
        if x[features[0].name].is_cuda:
            return self.embedding(x, features, squeeze_dim=squeeze_dim)
        return _embed_aten(self.embedding, x, features, squeeze_dim)

    def _project(self, input_user):
        return super()._project(input_user) if input_user.is_cuda else torch.matmul(input_user, self.convert_user_weight)

    def _normalize(self, t):
        return super()._normalize(t) if t.is_cuda else F.normalize(t, p=2, dim=-1)


class SINE(torch.nn.Module):
    """``torch_rechub.models.matching.SINE`` (sine.py:14-151): same constructor (feature NAMES, not Feature objects), parameter
    names (``item_embedding`` / ``concept_embedding`` / ``position_embedding``, ``w_1`` .. ``w_5``, ``w_k1``, ``w_k2``) and
    ``mode`` protocol.  Its three self-attentive stages are ``ops.sa_pool`` calls -- the concept vector z_u (pooled, heads
    summed), the per-intention weights P(t|k) (``attn`` only) and the next-intention vector over x_u_hat (pooled) -- and the
    history, target and negatives are ONE lookup of the item table through the gather kernel.  Top-k over the concepts, the
    softmaxes over K, the small einsums over K and the normalisations are ATen.  ``num_heads`` is kept; 1 is the only value for
    which the reference's forward runs (sine.py:123 reshapes [B, L, heads] to [-1, L]) and anything else raises here too."""

    def __init__(self, history_features, item_features, neg_item_features, num_items, embedding_dim, hidden_dim, num_concept,
                 num_intention, seq_max_len, num_heads=1, temperature=1.0):
        super().__init__()
        self.item_features = item_features
        self.history_features = history_features
        self.neg_item_features = neg_item_features
        self.temperature = temperature
        self.num_concept = num_concept
        self.num_intention = num_intention
        self.seq_max_len = seq_max_len
        self.num_heads = num_heads
        std = 1e-4
        self.item_embedding = torch.nn.Embedding(num_items, embedding_dim)
        torch.nn.init.normal_(self.item_embedding.weight, 0, std)
        self.concept_embedding = torch.nn.Embedding(num_concept, embedding_dim)
        torch.nn.init.normal_(self.concept_embedding.weight, 0, std)
        self.position_embedding = torch.nn.Embedding(seq_max_len, embedding_dim)
        torch.nn.init.normal_(self.position_embedding.weight, 0, std)
        self.w_1 = torch.nn.Parameter(torch.rand(embedding_dim, hidden_dim), requires_grad=True)
        self.w_2 = torch.nn.Parameter(torch.rand(hidden_dim, num_heads), requires_grad=True)
        self.w_3 = torch.nn.Parameter(torch.rand(embedding_dim, embedding_dim), requires_grad=True)
        self.w_k1 = torch.nn.Parameter(torch.rand(embedding_dim, hidden_dim), requires_grad=True)
        self.w_k2 = torch.nn.Parameter(torch.rand(hidden_dim, num_intention), requires_grad=True)
        self.w_4 = torch.nn.Parameter(torch.rand(embedding_dim, hidden_dim), requires_grad=True)
        self.w_5 = torch.nn.Parameter(torch.rand(hidden_dim, num_heads), requires_grad=True)
        self.mode = None

    def _items(self, x):
        """(history [B, L, D] or None, candidates [B, 1 (+ n_neg), D] or None): every id the mode needs in one lookup."""
        cols = []
        if self.mode != "item":
            cols.append(x[self.history_features[0]])
        if self.mode != "user":
            cols.append(x[self.item_features[0]].reshape(-1, 1))
            if self.mode != "item":
                neg = x[self.neg_item_features[0]]
                cols.append(neg.reshape(neg.shape[0], -1))
        ids = torch.cat([c.long() for c in cols], dim=1)
        emb = ops_position(self.item_embedding, ids) if ids.is_cuda else self.item_embedding(ids)
        n_hist = cols[0].shape[1] if self.mode != "item" else 0
        return (emb[:, :n_hist] if n_hist else None), (emb[:, n_hist:] if self.mode != "user" else None)

    def forward(self, x):
        hist_emb, cand_emb = self._items(x)
        user_embedding = self.user_tower(x, hist_emb)
        item_embedding = self.item_tower(x, cand_emb)
        if self.mode == "user":
            return user_embedding
        if self.mode == "item":
            return item_embedding
        return torch.mul(user_embedding, item_embedding).sum(dim=-1)                                       # [B, 1 + n_neg]

    def user_tower(self, x, hist_emb=None):
        if self.mode == "item":
            return None
        if self.num_heads != 1:
            raise ValueError("SINE: num_heads=%d; the reference's forward runs with 1 head only" % self.num_heads)
        if hist_emb is None:
            hist_emb = self._items(x)[0]
        einsum = torch.einsum
        hist = x[self.history_features[0]]
        x_u = hist_emb + self.position_embedding.weight.unsqueeze(0)                                      # [B, L, D]
        mask = (hist > 0).long()
        # sparse-interest extraction: the virtual concept vector z_u, its top concepts C^u
        z_u = ops.sa_pool(x_u, self.w_1, self.w_2, mask)[0].sum(dim=1)                                     # [B, D]
        s_u = einsum("be, te -> bt", z_u, self.concept_embedding.weight)
        top = torch.topk(s_u, self.num_intention)
        c_u = einsum("bk, bke -> bke", torch.sigmoid(top.values), F.embedding(top.indices, self.concept_embedding.weight))
        # intention assignment P(k|t), attention weighing P(t|k)
        p_u = torch.softmax(einsum("bse, bke -> bks", F.normalize(x_u @ self.w_3, dim=-1), F.normalize(c_u, p=2, dim=-1)), dim=1)
        a_concept_k = ops.sa_pool(x_u, self.w_k1, self.w_k2, mask, pool=False)[1]                          # [B, L, K]
        phi_u = einsum("bks, bse -> bke", p_u * a_concept_k.permute(0, 2, 1), x_u)
        # adaptive interest aggregation: the intention-aware input, the next intention, the aggregation weights
        x_u_hat = einsum("bks, bke -> bse", p_u, c_u)
        # as written: sine.py:120-125 calls F.normalize(t, -1), whose second positional argument is p -- the p = -1 norm over dim 1
        c_u_apt = F.normalize(ops.sa_pool(x_u_hat, self.w_4, self.w_5, mask)[0][:, 0], p=-1, dim=1)        # [B, D]
        e_u = torch.softmax(einsum("be, bke -> bk", c_u_apt, phi_u) / self.temperature, dim=1)
        v_u = einsum("bk, bke -> be", e_u, phi_u)
        if self.mode == "user":
            return v_u
        return v_u.unsqueeze(1)

    def item_tower(self, x, cand_emb=None):
        if self.mode == "user":
            return None
        if cand_emb is None:
            cand_emb = self._items(x)[1]
        if self.mode == "item":
            return cand_emb.squeeze(1)                                                                     # [B, D]
        return cand_emb                                                                                    # [B, 1 + n_neg, D]

    def gen_mask(self, x):
        return (x[self.history_features[0]] > 0).long()


class GRU4Rec(torch.nn.Module):
    """``torch_rechub.models.matching.GRU4Rec`` (gru4rec.py:16-87): the history runs through a bias-free stacked GRU
    (``user_params['num_layers']``, default 2) whose last layer's final state joins the user features in front of the user
    tower.  Same constructor, ``mode`` protocol and parameter names (``embedding.*``, ``gru.weight_*_l{k}``, ``user_mlp.*``);
    each GRU layer is one ``ops.gru`` call."""

    def __init__(self, user_features, history_features, item_features, neg_item_feature, user_params, temperature=1.0):
        super().__init__()
        self.user_features = user_features
        self.item_features = item_features
        self.history_features = history_features
        self.neg_item_feature = neg_item_feature
        self.temperature = temperature
        self.user_dims = sum([fea.embed_dim for fea in user_features + history_features])
        self.embedding = EmbeddingLayer(user_features + item_features + history_features)
        self.gru = GRU(input_size=history_features[0].embed_dim, hidden_size=history_features[0].embed_dim,
                       num_layers=user_params.get('num_layers', 2), batch_first=True, bias=False)
        self.user_mlp = MLP(self.user_dims, output_layer=False, **user_params)
        self.mode = None

    def forward(self, x):
        user_embedding = self.user_tower(x)
        item_embedding = self.item_tower(x)
        if self.mode == "user":
            return user_embedding
        if self.mode == "item":
            return item_embedding
        return torch.mul(user_embedding, item_embedding).sum(dim=1)                          # [B, D], as written

    def user_tower(self, x):
        if self.mode == "item":
            return None
        input_user = self.embedding(x, self.user_features, squeeze_dim=True)
        history_emb = self.embedding(x, self.history_features).squeeze(1)                    # [B, L, D]
        _, h_n = self.gru(history_emb)
        input_user = torch.cat([input_user, h_n[-1]], dim=-1)
        user_embedding = ops.l2_normalize(self.user_mlp(input_user).unsqueeze(1))            # [B, 1, D]
        if self.mode == "user":
            return user_embedding.squeeze(1)
        return user_embedding

    def item_tower(self, x):
        if self.mode == "user":
            return None
        pos_embedding = ops.l2_normalize(self.embedding(x, self.item_features, squeeze_dim=False))         # [B, 1, D]
        if self.mode == "item":
            return pos_embedding.squeeze(1)
        neg_embeddings = ops.l2_normalize(self.embedding(x, self.neg_item_feature, squeeze_dim=False).squeeze(1))
        return torch.cat((pos_embedding, neg_embeddings), dim=1)                                           # [B, 1 + n_neg, D]


class NARM(torch.nn.Module):
    """``torch_rechub.models.matching.NARM`` (narm.py:18-76): same constructor and ``state_dict`` keys (``item_emb.weight``,
    ``gru.*``, ``a_1``, ``a_2``, ``v``, ``b``).  The session lengths (non-zero ids per row; sessions are left-aligned) are
    counted on the device and handed to ``ops.gru`` as ``lengths``: no packing and no host copy (narm.py:49-50), so a step is
    capturable.  The reference's additive attention broadcasts the last state against the padded states in a way that needs
    one full-length session per batch; for every such batch the outputs agree.  The attention (Eq. 6-8) is one
    ``ops.additive_attn_pool`` call, the bilinear scoring (Eq. 10) is ``ops.linear``; dropout is ``ops.dropout`` (its Philox
    mask differs from torch's)."""

    def __init__(self, item_history_feature, hidden_dim, emb_dropout_p, session_rep_dropout_p):
        super(NARM, self).__init__()
        self.item_history_feature = item_history_feature
        self.item_emb = nn.Embedding(item_history_feature.vocab_size, item_history_feature.embed_dim, padding_idx=0)
        self.emb_dropout = nn.Dropout(emb_dropout_p)
        self.gru = GRU(input_size=item_history_feature.embed_dim, hidden_size=hidden_dim)
        self.a_1, self.a_2 = nn.Parameter(torch.randn(hidden_dim, hidden_dim)), nn.Parameter(torch.randn(hidden_dim, hidden_dim))
        self.v = nn.Parameter(torch.randn(hidden_dim, 1))
        self.session_rep_dropout = nn.Dropout(session_rep_dropout_p)
        self.b = nn.Parameter(torch.randn(item_history_feature.embed_dim, hidden_dim * 2))

    def _drop(self, layer, x):
        return ops.dropout(x, layer.p, True) if (self.training and layer.p > 0) else x

    def forward(self, input_dict):
        ids = input_dict[self.item_history_feature.name]
        ops._require_cuda(ids, "NARM input")
        value_mask = (ids != 0)
        lengths = value_mask.sum(dim=1)                                                      # stays on the device
        embs = self._drop(self.emb_dropout, ops_position(self.item_emb, ids))                # [B, L, E]
        # Eq. 1-4: hidden states of every step; positions beyond a session's length are 0, as pad_packed_sequence leaves them
        h, h_t = ops.gru(embs, self.gru.weight_ih_l0, self.gru.weight_hh_l0, self.gru.bias_ih_l0, self.gru.bias_hh_l0,
                         None, lengths)
        c_g = h_t                                                                            # Eq. 5 [B, H]
        # Eq. 6-8: similarity between the final state and every state, the masked weights and the weighted sum, one op
        c_l, _ = ops.additive_attn_pool(h, self.a_2, ops.linear(h_t, self.a_1), self.v[:, 0], value_mask, 0.0)
        c =self._drop(self.session_rep_dropout, torch.cat((c_g, c_l), dim=1))               # Eq. 9
        # Eq. 10 [B, V].  The table is also read by the lookup above, so autograd adds two gradients for it on the current stream:
        # it goes in as a view (not a leaf), which keeps this Linear's dW off the side stream (ops.config.dw_beside_lookup)
        return ops.linear(ops.linear(c, self.b), self.item_emb.weight.view_as(self.item_emb.weight))


class STAMP(torch.nn.Module):
    """``torch_rechub.models.matching.STAMP`` (stamp.py:15-83): same constructor, initialisation order and ``state_dict`` keys
    (``item_emb.weight``, ``w_0``, ``w_1_t``, ``w_2_t``, ``w_3_t``, ``b_a``, ``f_s.1.*``, ``f_t.1.*``); as there, the
    ``normal_`` initialisation of the table overwrites its padding row.  The session lengths (non-zero ids per row; sessions
    are left-aligned) are counted on the device; the last click is looked up at ``(lengths - 1).clamp_min(0)``, so an empty
    session does not fault (the reference's gather index is -1 there; its scores here are unspecified).  The general
    interest m_s (Eq. 2) is the masked pooling op, the attention (Eq. 7-8) one ``ops.additive_attn_pool`` call on the raw
    embeddings with ``eps = 1e-12`` (``F.normalize(p=1)`` over non-negative terms): masked positions get alpha = 0, which is
    the ``* value_mask`` of stamp.py:60.  ``f_s``, ``f_t`` and the catalogue scores are ``ops.linear``."""

    def __init__(self, item_history_feature, weight_std, emb_std):
        super(STAMP, self).__init__()
        self.item_history_feature = item_history_feature
        n_items, item_emb_dim = item_history_feature.vocab_size, item_history_feature.embed_dim
        self.item_emb = nn.Embedding(n_items, item_emb_dim, padding_idx=0)
        self.w_0 = nn.Parameter(torch.zeros(item_emb_dim, 1))
        self.w_1_t = nn.Parameter(torch.zeros(item_emb_dim, item_emb_dim))
        self.w_2_t = nn.Parameter(torch.zeros(item_emb_dim, item_emb_dim))
        self.w_3_t = nn.Parameter(torch.zeros(item_emb_dim, item_emb_dim))
        self.b_a = nn.Parameter(torch.zeros(item_emb_dim))
        for p in (self.w_0, self.w_1_t, self.w_2_t, self.w_3_t):
            nn.init.normal_(p, std=weight_std)
        self.f_s = nn.Sequential(nn.Tanh(), nn.Linear(item_emb_dim, item_emb_dim))
        self.f_t = nn.Sequential(nn.Tanh(), nn.Linear(item_emb_dim, item_emb_dim))
        self.emb_std = emb_std
        self.apply(self._init_module_weights)

    def _init_module_weights(self, module):
        if isinstance(module, nn.Linear):
            module.weight.data.normal_(std=self.emb_std)
            if module.bias is not None:
                module.bias.data.zero_()
        elif isinstance(module, nn.Embedding):
            module.weight.data.normal_(std=self.emb_std)

    def forward(self, input_dict):
        ids = input_dict[self.item_history_feature.name]
        ops._require_cuda(ids, "STAMP input")
        value_mask = (ids != 0)
        value_counts = value_mask.sum(dim=1, keepdim=True)                                   # [B, 1], stays on the device
        embs = ops_position(self.item_emb, ids)                                              # [B, L, D], raw rows
        # the latest click: its row is already among the looked-up ones (one lookup and one table gradient, not two)
        last = (value_counts - 1).clamp_min(0).unsqueeze(-1).expand(-1, 1, embs.shape[2])
        x_t = torch.gather(embs, 1, last).squeeze(1)                                         # [B, D]
        m_s = ops.pool(embs, value_mask, True, ops.DENOM_MASK, 0.0)                          # Eq. 2 [B, D]
        # Eq. 7-8: the context of the attention is what does not depend on the position
        ctx = ops.linear(x_t, self.w_2_t.t(), self.b_a) + ops.linear(m_s, self.w_3_t.t())
        m_a, _ = ops.additive_attn_pool(embs, self.w_1_t.t(), ctx, self.w_0[:, 0], value_mask, 1e-12)
        m_a = m_a + m_s
        h_s = ops.linear(torch.tanh(m_a), self.f_s[1].weight, self.f_s[1].bias)              # Eq. 3
        h_t = ops.linear(torch.tanh(x_t), self.f_t[1].weight, self.f_t[1].bias)              # Eq. 9
        # Eq. 4 [B, V]: the table goes in as a view, as in NARM (it is also read by the lookups above)
        return ops.linear(h_s * h_t, self.item_emb.weight.view_as(self.item_emb.weight))


class SRGNN(torch.nn.Module):
    """SR-GNN (Wu et al., AAAI 2019) as a rechub-style trainable session model beside ``STAMP``: ``SRGNN(item_history_feature,
    step=1)`` over ``recbole.SRGNNEncoder`` (RecBole's network, srgnn.py:126-217, with its ``state_dict`` keys under
    ``encoder.`` and its uniform +- 1 / sqrt(dim) initialisation).  ``forward(input_dict)`` returns the [B, V] catalogue
    scores.  The session lengths (non-zero ids per row; sessions are left-aligned) are counted on the device, the session
    graphs are built there (``ops.session_graph_torch``), so a training step copies nothing to the host; the propagation
    steps are ``ops.session_gnn_step_torch``."""

    def __init__(self, item_history_feature, step=1):
        super(SRGNN, self).__init__()
        from ...recbole.sequential import SRGNNEncoder
        self.item_history_feature = item_history_feature
        self.encoder = SRGNNEncoder(item_history_feature.vocab_size, item_history_feature.embed_dim, step)

    def forward(self, input_dict):
        ids = input_dict[self.item_history_feature.name]
        lengths = (ids != 0).sum(dim=1)                                                      # stays on the device
        return self.encoder.full_sort_scores(ids, lengths)


class Caser(torch.nn.Module):
    """Caser (Tang and Wang, WSDM 2018) as a rechub-style trainable session model beside ``SRGNN``: ``Caser(user_feature,
    item_history_feature, max_len, n_h=8, n_v=4, dropout_prob=0.4, reg_weight=1e-4)`` over ``recbole.CaserEncoder`` (RecBole's network,
    caser.py:42-155, with its ``state_dict`` keys under ``encoder.`` and its initialisation).  ``user_feature`` is a
    ``SparseFeature`` of the user ids, ``item_history_feature`` the ``SequenceFeature`` of the clicks and ``max_len`` the session
    length L the filters are built for.  ``forward(input_dict)`` returns the [B, V] catalogue scores; both convolution branches are
    one ``ops.caser_conv`` call."""

    def __init__(self, user_feature, item_history_feature, max_len, n_h=8, n_v=4, dropout_prob=0.4, reg_weight=1e-4):
        super(Caser, self).__init__()
        from ...recbole.sequential import CaserEncoder
        if user_feature.embed_dim != item_history_feature.embed_dim:
            raise ValueError("Caser: users and items share one width")
        self.user_feature, self.item_history_feature = user_feature, item_history_feature
        self.encoder = CaserEncoder(user_feature.vocab_size, item_history_feature.vocab_size, item_history_feature.embed_dim,
                                    int(max_len), n_h, n_v, dropout_prob, reg_weight)

    def forward(self, input_dict):
        return self.encoder.full_sort_scores(input_dict[self.user_feature.name], input_dict[self.item_history_feature.name])


class LightGCN(torch.nn.Module):
    """LightGCN (He et al., SIGIR 2020) as a rechub-style trainable matching model: ``LightGCN(user_feature, item_feature,
    graph, n_layers=3)`` over ``recbole.LightGCNEncoder`` (RecBole's network, lightgcn.py:60-151, with its ``state_dict`` keys
    under ``encoder.``).  ``user_feature`` / ``item_feature`` are ``SparseFeature``s (``vocab_size`` users / items of
    ``embed_dim``), ``graph`` the ``recbole.norm_adj`` of the training interactions.  ``forward(x)``: ``x[user_feature.name]``
    [B] and ``x[item_feature.name]`` [B, 1 + n_neg] (the positive first) -> [B, 1 + n_neg] inner-product scores of the
    propagated rows (``ops.pair_dot``); ``mode = "user"`` / ``"item"`` returns the propagated rows of the ids given.  The
    propagation is ``ops.graph_prop_mean``."""

    def __init__(self, user_feature, item_feature, graph, n_layers=3):
        super(LightGCN, self).__init__()
        from ...recbole.general import LightGCNEncoder
        if user_feature.embed_dim != item_feature.embed_dim:
            raise ValueError("LightGCN: users and items share one width")
        self.user_feature, self.item_feature = user_feature, item_feature
        self.encoder = LightGCNEncoder(user_feature.vocab_size, item_feature.vocab_size, user_feature.embed_dim, n_layers, graph)
        self.mode = None

    def forward(self, x):
        user_all, item_all = self.encoder()
        if self.mode == "user":
            return user_all[x[self.user_feature.name].long().reshape(-1)]
        if self.mode == "item":
            return item_all[x[self.item_feature.name].long().reshape(-1)]
        users = x[self.user_feature.name].long().reshape(-1)
        items = x[self.item_feature.name].long().reshape(users.shape[0], -1)
        u, v = user_all[users], item_all[items]                                              # [B, D], [B, 1 + n_neg, D]
        return ops.pair_dot(u, v) if u.is_cuda else (u.unsqueeze(1) * v).sum(-1)


class YoutubeSBC(torch.nn.Module):
    """Sampling-bias-corrected in-batch softmax (drop-in for ``torch_rechub.models.matching.youtube_sbc.YoutubeSBC``): same
    constructor, ``mode`` switch, ``index0`` / ``index1`` and parameter names.  The towers are the shared lookup and MLP; the
    scores -- user i against items i, i + 1, .., i + n_neg (mod B), cosine minus log(sample weight), over the temperature -- are
    one ``ops.inbatch_band_scores`` call: the reference's [B, B, D] broadcast of ``torch.cosine_similarity`` and its [B, B]
    matrix are never formed.

    A last batch of b < batch_size rows: the reference folds its stored ``index1`` twice, at batch_size when it is built and at
    b when the short batch arrives, so user i meets item ``fold_b(fold_batch_size(i + k))``.  While ``b + n_neg <= batch_size``
    that is ``(i + k) mod b`` and the band op serves it; beyond (the second fold then repeats an item) the same columns are
    gathered with plain torch ops, as a freshly built reference model returns them.  The reference also writes that fold back
    into ``index1`` through the slice view, which corrupts every later full batch; ``index0`` / ``index1`` are never changed
    here."""

    def __init__(self, user_features, item_features, sample_weight_feature, user_params, item_params, batch_size, n_neg=3,
                 temperature=1.0):
        super().__init__()
        self.user_features = user_features
        self.item_features = item_features
        self.sample_weight_feature = sample_weight_feature
        self.n_neg = n_neg
        self.temperature = temperature
        self.user_dims = sum([fea.embed_dim for fea in user_features])
        self.item_dims = sum([fea.embed_dim for fea in item_features])
        self.batch_size = batch_size
        self.embedding = EmbeddingLayer(user_features + item_features + sample_weight_feature)
        self.user_mlp = MLP(self.user_dims, output_layer=False, **user_params)
        self.item_mlp = MLP(self.item_dims, output_layer=False, **item_params)
        self.mode = None
        # in-batch sampling index, kept as the reference builds it (the scores do not read it on a full batch)
        self.index0 = np.repeat(np.arange(batch_size), n_neg + 1)
        self.index1 = np.concatenate([np.arange(i, i + n_neg + 1) for i in range(batch_size)])
        self.index1[np.where(self.index1 >= batch_size)] -= batch_size

    def forward(self, x):
        user_embedding = self.user_tower(x)
        item_embedding = self.item_tower(x)
        if self.mode == "user":
            return user_embedding
        if self.mode == "item":
            return item_embedding
        if all(isinstance(f, DenseFeature) for f in self.sample_weight_feature):
            # dense values need no lookup launch: the columns the squeezed gather would lay out
            sample_weight = torch.cat([x[f.name].float().unsqueeze(1) for f in self.sample_weight_feature], dim=1).squeeze(1)
        else:
            sample_weight = _embed_any(self.embedding, x, self.sample_weight_feature, True).squeeze(1)       # [B]
        b = user_embedding.shape[0]
        if b == self.batch_size or b + self.n_neg <= self.batch_size:
            return ops.inbatch_band_scores(user_embedding, item_embedding, self.n_neg, weight=sample_weight,
                                           temperature=self.temperature)
        if b > self.batch_size:
            raise ValueError("YoutubeSBC: a batch of %d rows, the model was built for batch_size = %d" % (b, self.batch_size))
        # the short batch whose band crosses batch_size: the reference's doubly folded columns, on a copy
        index1 = self.index1[:b * (self.n_neg + 1)].copy()
        index1[np.where(index1 >= b)] -= b
        cols = torch.as_tensor(index1, device=user_embedding.device).view(b, self.n_neg + 1)
        items = item_embedding[cols]                                                                        # [b, n_neg + 1, D]
        pred = torch.cosine_similarity(user_embedding.unsqueeze(1), items, dim=2)
        return (pred - torch.log(sample_weight)[cols]) / self.temperature

    def user_tower(self, x):
        if self.mode == "item":
            return None
        return _mlp(self.user_mlp, _embed_any(self.embedding, x, self.user_features, True))

    def item_tower(self, x):
        if self.mode == "user":
            return None
        return _mlp(self.item_mlp, _embed_any(self.embedding, x, self.item_features, True))


def _normalize_rows(x):
    return ops.l2_normalize(x) if x.is_cuda else F.normalize(x, p=2, dim=1)


def _row_dot(u, v):
    return ops.pair_dot(u, v).squeeze(1) if u.is_cuda else torch.mul(u, v).sum(dim=1)


class FaceBookDSSM(torch.nn.Module):
    """Pair-wise two-tower trained with a hinge loss (drop-in for ``torch_rechub.models.matching.dssm_facebook.FaceBookDSSM``):
    same constructor, ``mode`` switch, outputs ``(pos_score, neg_score)`` and parameter names.  Both towers end in
    ``ops.l2_normalize``, the two scores are ``ops.pair_dot``; ``mode="item"`` returns the positive item's embedding before the
    normalisation, as the reference does."""

    def __init__(self, user_features, pos_item_features, neg_item_features, user_params, item_params, temperature=1.0):
        super().__init__()
        self.user_features = user_features
        self.pos_item_features = pos_item_features
        self.neg_item_features = neg_item_features
        self.temperature = temperature
        self.user_dims = sum([fea.embed_dim for fea in user_features])
        self.item_dims = sum([fea.embed_dim for fea in pos_item_features])
        self.embedding = EmbeddingLayer(user_features + pos_item_features + neg_item_features)
        self.user_mlp = MLP(self.user_dims, output_layer=False, **user_params)
        self.item_mlp = MLP(self.item_dims, output_layer=False, **item_params)
        self.mode = None

    def forward(self, x):
        user_embedding = self.user_tower(x)
        pos_item_embedding, neg_item_embedding = self.item_tower(x)
        if self.mode == "user":
            return user_embedding
        if self.mode == "item":
            return pos_item_embedding
        return _row_dot(user_embedding, pos_item_embedding), _row_dot(user_embedding, neg_item_embedding)

    def user_tower(self, x):
        if self.mode == "item":
            return None
        input_user = _embed_any(self.embedding, x, self.user_features, True)
        return _normalize_rows(_mlp(self.user_mlp, input_user))

    def item_tower(self, x):
        if self.mode == "user":
            return None, None
        input_item_pos = _embed_any(self.embedding, x, self.pos_item_features, True)
        if self.mode == "item":
            return _mlp(self.item_mlp, input_item_pos), None
        input_item_neg = _embed_any(self.embedding, x, self.neg_item_features, True)
        pos_embedding, neg_embedding = _mlp(self.item_mlp, input_item_pos), _mlp(self.item_mlp, input_item_neg)
        return _normalize_rows(pos_embedding), _normalize_rows(neg_embedding)
