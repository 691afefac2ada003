"""``AttLayer``, ``MLPLayers``, ``activation_layer``, ``Dice`` and ``SequenceAttLayer`` of RecBole
(third_party/recbole/model/layers.py:30-124, 236-354)."""
import numpy as np
import torch
from torch import nn
from torch.nn.init import normal_

from .. import ops


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


def _run_modules(mods, x):
    """An ``nn.Sequential``'s modules over ``x``: the Linears on ``ops.linear`` for GPU tensors, everything else as it is."""
    for m in mods:
        x = ops.linear(x, m.weight, m.bias) if (type(m) is nn.Linear and x.is_cuda) else m(x)
    return x


class MLPLayers(nn.Module):
    """RecBole's MLP: per layer Dropout, Linear, optional BatchNorm1d, optional activation, in the reference's module order
    (``mlp_layers.<i>.weight`` agree).  The Linears run on ``ops.linear`` for GPU tensors."""

    def __init__(self, layers, dropout=0.0, activation="relu", bn=False, init_method=None):
        super(MLPLayers, self).__init__()
        self.layers = layers
        self.dropout = dropout
        self.activation = activation
        self.use_bn = bn
        self.init_method = init_method

        mlp_modules = []
        for input_size, output_size in zip(self.layers[:-1], self.layers[1:]):
            mlp_modules.append(nn.Dropout(p=self.dropout))
            mlp_modules.append(nn.Linear(input_size, output_size))
            if self.use_bn:
                mlp_modules.append(nn.BatchNorm1d(num_features=output_size))
            activation_func = activation_layer(self.activation, output_size)
            if activation_func is not None:
                mlp_modules.append(activation_func)

        self.mlp_layers = nn.Sequential(*mlp_modules)
        if self.init_method is not None:
            self.apply(self.init_weights)

    def init_weights(self, module):
        if isinstance(module, nn.Linear):
            if self.init_method == "norm":
                normal_(module.weight.data, 0, 0.01)
            if module.bias is not None:
                module.bias.data.fill_(0.0)

    def forward(self, input_feature):
        return _run_modules(self.mlp_layers, input_feature)


def activation_layer(activation_name="relu", emb_dim=None):
    """The activation module of a name ('sigmoid', 'tanh', 'relu', 'leakyrelu', 'dice', 'none'), of a Module class, or None."""
    activation = None
    if activation_name is None:
        activation = None
    elif isinstance(activation_name, str):
        name = activation_name.lower()
        if name == "sigmoid":
            activation = nn.Sigmoid()
        elif name == "tanh":
            activation = nn.Tanh()
        elif name == "relu":
            activation = nn.ReLU()
        elif name == "leakyrelu":
            activation = nn.LeakyReLU()
        elif name == "dice":
            activation = Dice(emb_dim)
        elif name == "none":
            activation = None
    elif issubclass(activation_name, nn.Module):
        activation = activation_name()
    else:
        raise NotImplementedError("activation function {} is not implemented".format(activation_name))
    return activation


class Dice(nn.Module):
    """RecBole's Dice: ``p = sigmoid(s)``, ``alpha (1 - p) s + p s`` with ``alpha`` a plain zero tensor (not a parameter, not in
    the ``state_dict``, no batch statistics) -- not the Dice of the ranking zoo."""

    def __init__(self, emb_size):
        super(Dice, self).__init__()
        self.sigmoid = nn.Sigmoid()
        self.alpha = torch.zeros((emb_size,))

    def forward(self, score):
        self.alpha = self.alpha.to(score.device)
        score_p = self.sigmoid(score)
        return self.alpha * (1 - score_p) * score + score_p * score


class SequenceAttLayer(nn.Module):
    """DIN's / DIEN's attention over a sequence: an MLP over ``[q, k, q - k, q k]`` and a Linear to one score per position,
    the positions at and beyond ``keys_length`` filled with ``-inf`` (``softmax_stag``) or 0, ``/ sqrt(E)``, the optional
    softmax; ``return_seq_weight`` False multiplies the weights into the keys.  ``queries`` [B, E], ``keys`` [B, T, E],
    ``keys_length`` [B] -> [B, 1, T] or [B, 1, E].  For GPU tensors the first Linear is ``ops.din_scores`` (same column order,
    no [B, T, 4E] tensor) where that op takes the layout (``ops.din_scores_supported``) and the Linears are ``ops.linear``.
    The mask is built from ``keys_length`` on the device; ``mask_mat`` is kept as an attribute only."""

    def __init__(self, mask_mat, att_hidden_size=(80, 40), activation="sigmoid", softmax_stag=False, return_seq_weight=True):
        super(SequenceAttLayer, self).__init__()
        self.att_hidden_size = att_hidden_size
        self.activation = activation
        self.softmax_stag = softmax_stag
        self.return_seq_weight = return_seq_weight
        self.mask_mat = mask_mat
        self.att_mlp_layers = MLPLayers(self.att_hidden_size, activation=self.activation, bn=False)
        self.dense = nn.Linear(self.att_hidden_size[-1], 1)

    def _mlp(self, queries, keys):
        B, T, E = keys.shape
        mods = list(self.att_mlp_layers.mlp_layers)
        if (keys.is_cuda and len(mods) >= 2 and type(mods[0]) is nn.Dropout and (mods[0].p == 0 or not mods[0].training)
                and type(mods[1]) is nn.Linear and ops.din_scores_supported(keys, queries, mods[1].weight)):
            first = ops.din_scores(keys, queries, mods[1].weight, mods[1].bias).view(B, T, -1)
            return _run_modules(mods[2:], first)
        q = queries.unsqueeze(1).expand(B, T, E)
        return _run_modules(mods, torch.cat([q, keys, q - keys, q * keys], dim=-1))

    def forward(self, queries, keys, keys_length):
        embedding_size = queries.shape[-1]
        hist_len = keys.shape[1]
        output = _run_modules([self.dense], self._mlp(queries, keys))          # [B, T, 1]
        output = torch.transpose(output, -1, -2).squeeze(1)                    # [B, T]
        mask = torch.arange(hist_len, device=keys.device).view(1, -1) >= keys_length.to(keys.device).unsqueeze(1)
        mask_value = -np.inf if self.softmax_stag else 0.0
        output = output.masked_fill(mask=mask, value=mask_value)
        output = output.unsqueeze(1)
        output = output / (embedding_size ** 0.5)
        if self.softmax_stag:
            output = torch.softmax(output, dim=2)                              # [B, 1, T]
        if not self.return_seq_weight:
            output = torch.matmul(output, keys)                                # [B, 1, E]
        return output
