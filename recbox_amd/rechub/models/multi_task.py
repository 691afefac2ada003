"""Multi-task ranking models (drop-ins for ``torch_rechub.models.multi_task``, the reference's
third_party/rechub/models/multi_task/): SharedBottom (shared_bottom.py:14-45), ESMM (esmm.py:15-48),
MMOE (mmoe.py:15-58), PLE with CGC (ple.py:15-130) and AITM with its AttentionLayer (aitm.py:16-84).  Same constructors,
attribute names and ``state_dict`` keys; the reference is reproduced as written, oddities included.

The lookups, towers, BatchNorm and prediction heads are the layers of ``..basic.layers``.  The step these models are named
after -- mixing expert outputs under per-task softmax gates -- is ``ops.expert_mix`` (csrc/rbx_mix.hip): one launch forward
and one backward that read every expert row once for all gates, on the experts as the separate tensors they are (no
``torch.cat``).  CPU tensors run the same models in ATen."""
import torch
import torch.nn as nn

from ... import dense, ops
from ..basic.features import DenseFeature, SequenceFeature, SparseFeature
from ..basic.layers import MLP, EmbeddingLayer, PredictionLayer

__all__ = ["SharedBottom", "ESMM", "MMOE", "PLE", "CGC", "AITM", "AttentionLayer"]


def _on_gpu(x, features):
    return x[features[0].name].is_cuda


def _embed(layer, x, features, squeeze_dim):
    """``layer(x, features, squeeze_dim)``; for CPU tensors the reference's lines in ATen (one-hot features, sum / mean /
    concat sequence features with the id != padding mask, dense values)."""
    if _on_gpu(x, features):
        return layer(x, features, squeeze_dim=squeeze_dim)
    sparse, dense_values = [], []
    for fea in features:
        if isinstance(fea, DenseFeature):
            dense_values.append(x[fea.name].float().unsqueeze(1))
            continue
        table = layer.embed_dict[fea.name if fea.shared_with is None else fea.shared_with]
        ids = x[fea.name].long()
        if isinstance(fea, SparseFeature):
            sparse.append(table(ids).unsqueeze(1))
        elif isinstance(fea, SequenceFeature):
            if fea.pooling not in ("sum", "mean", "concat"):
                raise ValueError("Sequence pooling method supports only pooling in %s, got %s." % (["sum", "mean"], fea.pooling))
            rows = table(ids)
            if fea.pooling != "concat":
                mask = (ids != (fea.padding_idx if fea.padding_idx is not None else -1)).float()
                pooled = torch.bmm(mask.unsqueeze(1), rows).squeeze(1)
                if fea.pooling == "mean":
                    pooled = pooled / (mask.sum(dim=-1, keepdim=True) + 1e-16)
                rows = pooled
            sparse.append(rows.unsqueeze(1))
        else:
            raise ValueError("unknown feature class %s" % type(fea).__name__)
    if squeeze_dim:
        if not sparse and not dense_values:
            raise ValueError("The input features can note be empty")
        parts = ([torch.cat(sparse, dim=1).flatten(start_dim=1)] if sparse else []) + dense_values
        return torch.cat(parts, dim=1)
    if not sparse:
        raise ValueError("If keep the original shape:[batch_size, num_features, embed_dim], expected %s in feature list, got %s"
                         % ("SparseFeatures", features))
    return torch.cat(sparse, dim=1)


def _mlp(mlp, x):
    """``mlp(x)``: the dense path on the GPU, the plain ``nn.Sequential`` for CPU tensors."""
    return mlp(x) if x.is_cuda else mlp.mlp(x)


def _linear(x, layer):
    return ops.linear(x, layer.weight, layer.bias) if x.is_cuda else layer(x)


def _gate_logits(gate, x):
    """(gate input of ``ops.expert_mix``, softmax flag) for a gate ``MLP``.  A gate of the form the reference builds --
    Linear, BatchNorm1d, Softmax(dim=1), Dropout -- whose dropout is inactive hands the post-BatchNorm logits over and leaves
    the softmax to the mixing kernel; any other gate runs as it stands and its output is used as the weights."""
    mods = list(gate.mlp)
    if (len(mods) == 4 and type(mods[0]) is nn.Linear and type(mods[1]) is nn.BatchNorm1d and type(mods[2]) is nn.Softmax
            and mods[2].dim == 1 and type(mods[3]) is nn.Dropout and (mods[3].p == 0 or not mods[3].training)):
        head = mods[:2]
        return (dense.run_sequential(head, x) if x.is_cuda else mods[1](mods[0](x))), True
    return _mlp(gate, x), False


def _mix(experts, gate_mlps, gate_inputs, select):
    """One ``ops.expert_mix`` call for all gates of a layer.  Gates of both kinds in one layer (a hand-built model): the
    soft-maxed ones are applied here, so that the call takes weights throughout."""
    pairs = [_gate_logits(g, xi) for g, xi in zip(gate_mlps, gate_inputs)]
    softmax = all(flag for _, flag in pairs)
    zs = [z if (softmax or not flag) else torch.softmax(z, dim=1) for z, flag in pairs]
    return ops.expert_mix(experts, zs, select, softmax=softmax)


class SharedBottom(nn.Module):
    """Shared-bottom multi-task model: one bottom MLP, one tower and prediction head per task.  It has no kernel of its own:
    lookup, MLPs and heads are the shared layers."""

    def __init__(self, features, task_types, bottom_params, tower_params_list):
        super().__init__()
        self.features = features
        self.task_types = task_types
        self.embedding = EmbeddingLayer(features)
        self.bottom_dims = sum([fea.embed_dim for fea in features])
        self.bottom_mlp = MLP(self.bottom_dims, **{**bottom_params, **{"output_layer": False}})
        self.towers = nn.ModuleList(MLP(bottom_params["dims"][-1], **tower_params_list[i]) for i in range(len(task_types)))
        self.predict_layers = nn.ModuleList(PredictionLayer(task_type) for task_type in task_types)

    def forward(self, x):
        input_bottom = _embed(self.embedding, x, self.features, True)
        h = _mlp(self.bottom_mlp, input_bottom)
        ys = [predict_layer(_mlp(tower, h)) for tower, predict_layer in zip(self.towers, self.predict_layers)]
        return torch.cat(ys, dim=1)


class ESMM(nn.Module):
    """Entire Space Multi-Task Model: field-wise sum pooling of the user and the item embeddings, a CVR and a CTR tower.  It
    has no kernel of its own.  As in the reference (esmm.py:45) the third column is ``cvr_pred * cvr_pred``."""

    def __init__(self, user_features, item_features, cvr_params, ctr_params):
        super().__init__()
        self.user_features = user_features
        self.item_features = item_features
        self.embedding = EmbeddingLayer(user_features + item_features)
        self.tower_dims = user_features[0].embed_dim + item_features[0].embed_dim
        self.tower_cvr = MLP(self.tower_dims, **cvr_params)
        self.tower_ctr = MLP(self.tower_dims, **ctr_params)

    def forward(self, x):
        embed_user_features = _embed(self.embedding, x, self.user_features, False).sum(dim=1)
        embed_item_features = _embed(self.embedding, x, self.item_features, False).sum(dim=1)
        input_tower = torch.cat((embed_user_features, embed_item_features), dim=1)
        cvr_pred = torch.sigmoid(_mlp(self.tower_cvr, input_tower))
        ctr_pred = torch.sigmoid(_mlp(self.tower_ctr, input_tower))
        ctcvr_pred = torch.mul(cvr_pred, cvr_pred)
        return torch.cat([cvr_pred, ctr_pred, ctcvr_pred], dim=1)


class MMOE(nn.Module):
    """Multi-gate Mixture-of-Experts: ``n_expert`` expert MLPs over the embedded input, one softmax gate per task; all tasks'
    mixtures come out of one ``ops.expert_mix`` call on the expert outputs as separate tensors."""

    def __init__(self, features, task_types, n_expert, expert_params, tower_params_list):
        super().__init__()
        self.features = features
        self.task_types = task_types
        self.n_task = len(task_types)
        self.n_expert = n_expert
        self.embedding = EmbeddingLayer(features)
        self.input_dims = sum([fea.embed_dim for fea in features])
        self.experts = nn.ModuleList(MLP(self.input_dims, output_layer=False, **expert_params) for i in range(self.n_expert))
        self.gates = nn.ModuleList(
            MLP(self.input_dims, output_layer=False, **{"dims": [self.n_expert], "activation": "softmax"})
            for i in range(self.n_task))
        self.towers = nn.ModuleList(MLP(expert_params["dims"][-1], **tower_params_list[i]) for i in range(self.n_task))
        self.predict_layers = nn.ModuleList(PredictionLayer(task_type) for task_type in task_types)

    def forward(self, x):
        embed_x = _embed(self.embedding, x, self.features, True)
        expert_outs = [_mlp(expert, embed_x) for expert in self.experts]
        pooled = _mix(expert_outs, self.gates, [embed_x] * self.n_task, None)
        ys = [predict_layer(_mlp(tower, h)) for h, tower, predict_layer in zip(pooled, self.towers, self.predict_layers)]
        return torch.cat(ys, dim=1)


class CGC(nn.Module):
    """Customized Gate Control layer of PLE: per task ``n_expert_specific`` experts of its own, ``n_expert_shared`` shared
    ones; task i's gate mixes its own experts and the shared ones, and below the last level a further gate mixes all of
    them.  One ``ops.expert_mix`` call per layer serves every gate."""

    def __init__(self, cur_level, n_level, n_task, n_expert_specific, n_expert_shared, input_dims, expert_params):
        super().__init__()
        self.cur_level = cur_level
        self.n_level = n_level
        self.n_task = n_task
        self.n_expert_specific = n_expert_specific
        self.n_expert_shared = n_expert_shared
        self.n_expert_all = n_expert_specific * self.n_task + n_expert_shared
        input_dims = input_dims if cur_level == 1 else expert_params["dims"][-1]
        self.experts_specific = nn.ModuleList(
            MLP(input_dims, output_layer=False, **expert_params) for _ in range(self.n_task * self.n_expert_specific))
        self.experts_shared = nn.ModuleList(
            MLP(input_dims, output_layer=False, **expert_params) for _ in range(self.n_expert_shared))
        self.gates_specific = nn.ModuleList(
            MLP(input_dims, **{"dims": [self.n_expert_specific + self.n_expert_shared], "activation": "softmax",
                               "output_layer": False}) for _ in range(self.n_task))
        if cur_level < n_level:
            self.gate_shared = MLP(input_dims, **{"dims": [self.n_expert_all], "activation": "softmax", "output_layer": False})

    def forward(self, x_list):
        s = self.n_expert_specific
        outs = [_mlp(expert, x_list[i // s]) for i, expert in enumerate(self.experts_specific)]
        outs += [_mlp(expert, x_list[-1]) for expert in self.experts_shared]
        shared = list(range(self.n_task * s, self.n_expert_all))
        select = [list(range(i * s, (i + 1) * s)) + shared for i in range(self.n_task)]
        gates, inputs = list(self.gates_specific), list(x_list[:self.n_task])
        if self.cur_level < self.n_level:
            select.append(list(range(self.n_expert_all)))
            gates.append(self.gate_shared)
            inputs.append(x_list[-1])
        return list(_mix(outs, gates, inputs, select))


class PLE(nn.Module):
    """Progressive Layered Extraction: ``n_level`` CGC layers, then per task a tower and a prediction head.  As in the
    reference (ple.py:40-41) the towers are built with ``output_layer=False``."""

    def __init__(self, features, task_types, n_level, n_expert_specific, n_expert_shared, expert_params, tower_params_list):
        super().__init__()
        self.features = features
        self.n_task = len(task_types)
        self.task_types = task_types
        self.n_level = n_level
        self.input_dims = sum([fea.embed_dim for fea in features])
        self.embedding = EmbeddingLayer(features)
        self.cgc_layers = nn.ModuleList(
            CGC(i + 1, n_level, self.n_task, n_expert_specific, n_expert_shared, self.input_dims, expert_params)
            for i in range(n_level))
        self.towers = nn.ModuleList(
            MLP(expert_params["dims"][-1], output_layer=False, **tower_params_list[i]) for i in range(self.n_task))
        self.predict_layers = nn.ModuleList(PredictionLayer(task_type) for task_type in task_types)

    def forward(self, x):
        embed_x = _embed(self.embedding, x, self.features, True)
        ple_inputs = [embed_x] * (self.n_task + 1)
        ple_outs = []
        for i in range(self.n_level):
            ple_outs = self.cgc_layers[i](ple_inputs)
            ple_inputs = ple_outs
        ys = [predict_layer(_mlp(tower, h)) for h, tower, predict_layer in zip(ple_outs, self.towers, self.predict_layers)]
        return torch.cat(ys, dim=1)


class AttentionLayer(nn.Module):
    """AITM's attention for information transfer: x [B, 2, dim] -> [B, dim].  q / k / v are three GEMMs over the [2B, dim]
    rows; the two scores per sample, scaled by 1 / sqrt(dim), are the gate of ``ops.expert_mix`` over the two interleaved rows
    of V, read in place (E = 2, T = 1, row stride 2 dim)."""

    def __init__(self, dim=32):
        super().__init__()
        self.dim = dim
        self.q_layer = nn.Linear(dim, dim, bias=False)
        self.k_layer = nn.Linear(dim, dim, bias=False)
        self.v_layer = nn.Linear(dim, dim, bias=False)
        self.softmax = nn.Softmax(dim=1)

    def forward(self, x):
        rows = x.reshape(-1, self.dim)
        Q, K = _linear(rows, self.q_layer), _linear(rows, self.k_layer)
        V = _linear(rows, self.v_layer).view(-1, 2, self.dim)
        a = torch.sum(torch.mul(Q, K), -1).view(-1, 2) / self.dim ** 0.5
        return ops.expert_mix([V[:, 0], V[:, 1]], [a], softmax=True)[0]


class AITM(nn.Module):
    """Adaptive Information Transfer Multi-task framework: a bottom MLP and a tower per (binary) task; task i > 0 attends over
    its own bottom output and the previous task's transferred information (``AttentionLayer``)."""

    def __init__(self, features, n_task, bottom_params, tower_params_list):
        super().__init__()
        self.features = features
        self.n_task = n_task
        self.input_dims = sum([fea.embed_dim for fea in features])
        self.embedding = EmbeddingLayer(features)
        self.bottoms = nn.ModuleList(MLP(self.input_dims, output_layer=False, **bottom_params) for i in range(self.n_task))
        self.towers = nn.ModuleList(MLP(bottom_params["dims"][-1], **tower_params_list[i]) for i in range(self.n_task))
        self.info_gates = nn.ModuleList(
            MLP(bottom_params["dims"][-1], output_layer=False, dims=[bottom_params["dims"][-1]]) for i in range(self.n_task - 1))
        self.aits = nn.ModuleList(AttentionLayer(bottom_params["dims"][-1]) for _ in range(self.n_task - 1))

    def forward(self, x):
        embed_x = _embed(self.embedding, x, self.features, True)
        input_towers = [_mlp(self.bottoms[i], embed_x) for i in range(self.n_task)]
        for i in range(1, self.n_task):
            info = _mlp(self.info_gates[i - 1], input_towers[i - 1]).unsqueeze(1)
            ait_input = torch.cat([input_towers[i].unsqueeze(1), info], dim=1)
            input_towers[i] = self.aits[i - 1](ait_input)
        ys = [torch.sigmoid(_mlp(tower, h)) for h, tower in zip(input_towers, self.towers)]
        return torch.cat(ys, dim=1)
