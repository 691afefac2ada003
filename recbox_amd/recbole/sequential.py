"""The layers of RecBole's DIEN (third_party/recbole/model/sequential_recommender/dien.py:193-521): ``AGRUCell``, ``AUGRUCell``,
``DynamicRNN``, ``InterestExtractorNetwork`` and ``InterestEvolvingLayer``, with the reference's constructors, attribute names
and ``state_dict`` keys.  For GPU tensors the attention-gated recurrence is ``ops.att_gru`` (one launch each way,
csrc/rbx_gru.hip), the plain GRUs are ``ops.gru`` with the lengths read on the device, and nothing is packed or copied to
the host; for CPU tensors the same arithmetic runs in plain ATen.  RecBole's ``DIEN(config, dataset)`` model,
``ContextSeqEmbLayer`` and ``calculate_loss`` are not mirrored (``rechub.models.ranking.DIEN`` is the trainable model)."""
import math

import torch
import torch.nn.functional as F
from torch import nn
from torch.nn.utils.rnn import PackedSequence, pack_padded_sequence, pad_packed_sequence

from .. import ops
from .layers import MLPLayers, SequenceAttLayer


def _masked_walk(step, x, h, lengths):
    """``h = step(t, h)`` over the positions of ``x`` [B, L, .] with packed-sequence semantics -> (out [B, L, H], h_n)."""
    outs = []
    for t in range(x.shape[1]):
        new = step(t, h)
        if lengths is not None:
            act = (lengths > t).unsqueeze(1)
            h = torch.where(act, new, h)
            outs.append(torch.where(act, new, torch.zeros_like(new)))
        else:
            h = new
            outs.append(new)
    return torch.stack(outs, dim=1), h


def _gru_padded(gru, x, lengths):
    """One-layer batch-first ``nn.GRU`` as parameter holder over padded ``x`` [B, L, I] -> (out [B, L, H], h_n [B, H])."""
    w_ih, w_hh = gru.weight_ih_l0, gru.weight_hh_l0
    b_ih, b_hh = (gru.bias_ih_l0, gru.bias_hh_l0) if gru.bias else (None, None)
    if x.is_cuda:
        return ops.gru(x, w_ih, w_hh, b_ih, b_hh, None, lengths)
    H = gru.hidden_size
    gi = F.linear(x, w_ih, b_ih)

    def step(t, h):
        gh = F.linear(h, w_hh, b_hh)
        r = torch.sigmoid(gi[:, t, :H] + gh[:, :H])
        z = torch.sigmoid(gi[:, t, H:2 * H] + gh[:, H:2 * H])
        n = torch.tanh(gi[:, t, 2 * H:] + r * gh[:, 2 * H:])
        return (1 - z) * n + z * h
    return _masked_walk(step, x, x.new_zeros(x.shape[0], H), lengths)


class _AttCell(nn.Module):
    """What AGRUCell and AUGRUCell share: the parameters (rows ordered r, u, n; ``torch.randn`` weights, zero biases) and
    one step in ATen."""
    cell = None

    def __init__(self, input_size, hidden_size, bias=True):
        super(_AttCell, self).__init__()
        self.input_size = input_size
        self.hidden_size = hidden_size
        self.bias = bias
        self.weight_ih = nn.Parameter(torch.randn(3 * hidden_size, input_size))
        self.weight_hh = nn.Parameter(torch.randn(3 * hidden_size, hidden_size))
        if self.bias:
            self.bias_ih = nn.Parameter(torch.zeros(3 * hidden_size))
            self.bias_hh = nn.Parameter(torch.zeros(3 * hidden_size))
        else:
            self.register_parameter("bias_ih", None)
            self.register_parameter("bias_hh", None)

    def forward(self, input, hidden_output, att_score):
        gi = F.linear(input, self.weight_ih, self.bias_ih)
        gh = F.linear(hidden_output, self.weight_hh, self.bias_hh)
        i_r, i_u, i_h = gi.chunk(3, 1)
        h_r, h_u, h_h = gh.chunk(3, 1)
        reset_gate = torch.sigmoid(i_r + h_r)
        new_state = torch.tanh(i_h + reset_gate * h_h)
        att_score = att_score.view(-1, 1)
        if self.cell == "AUGRU":
            att_score = att_score * torch.sigmoid(i_u + h_u)
        return (1 - att_score) * hidden_output + att_score * new_state


class AGRUCell(_AttCell):
    """Attention based GRU: the score replaces the update gate, ``h' = (1 - a) h + a n`` (the u rows are unused)."""
    cell = "AGRU"


class AUGRUCell(_AttCell):
    """GRU with attentional update gate: ``c = a u``, ``h' = (1 - c) h + c n``."""
    cell = "AUGRU"


class DynamicRNN(nn.Module):
    """The attention-gated recurrence over a cell's parameters (``rnn.weight_ih`` ...).  ``forward`` takes the packed pair
    exactly as the reference does -- it unpacks, runs ``forward_padded`` and repacks, which reads the lengths on the host: for
    drop-in use, not capturable.  ``forward_padded(keys, att, lengths)`` is the padded form the layers below call."""

    def __init__(self, input_size, hidden_size, bias=True, gru="AGRU"):
        super(DynamicRNN, self).__init__()
        self.input_size = input_size
        self.hidden_size = hidden_size
        if gru == "AGRU":
            self.rnn = AGRUCell(input_size, hidden_size, bias)
        elif gru == "AUGRU":
            self.rnn = AUGRUCell(input_size, hidden_size, bias)

    def forward_padded(self, keys, att_scores, keys_length=None, hidden_output=None):
        """``keys`` [B, L, I], ``att_scores`` [B, L], ``keys_length`` [B] or None -> (out [B, L, H], h_n [B, H])."""
        cell = self.rnn
        if keys.is_cuda:
            return ops.att_gru(keys, att_scores, cell.weight_ih, cell.weight_hh, cell.bias_ih, cell.bias_hh, hidden_output,
                               keys_length, cell=cell.cell)
        h = hidden_output if hidden_output is not None else keys.new_zeros(keys.shape[0], self.hidden_size)
        att_scores = att_scores.reshape(keys.shape[0], keys.shape[1])
        return _masked_walk(lambda t, h: cell(keys[:, t], h, att_scores[:, t]), keys, h, keys_length)

    def forward(self, input, att_scores=None, hidden_output=None):
        if not isinstance(input, PackedSequence) or not isinstance(att_scores, PackedSequence):
            raise NotImplementedError("DynamicRNN only supports packed input and att_scores")
        keys, lengths = pad_packed_sequence(input, batch_first=True)
        att, _ = pad_packed_sequence(att_scores, batch_first=True)
        if hidden_output is not None and input.unsorted_indices is not None:
            hidden_output = hidden_output[input.unsorted_indices]          # the reference's rows follow the packed order
        out, _ = self.forward_padded(keys, att, lengths.to(keys.device), hidden_output)
        return pack_padded_sequence(out, lengths, batch_first=True, enforce_sorted=input.sorted_indices is None)


class InterestExtractorNetwork(nn.Module):
    """The interest extractor: a GRU over the behaviour sequence (``gru``: an ``nn.GRU`` as parameter holder, the compute on
    ``ops.gru`` with the lengths on the device) and the auxiliary loss of the next behaviour against a negative one."""

    def __init__(self, input_size, hidden_size, mlp_size):
        super(InterestExtractorNetwork, self).__init__()
        self.gru = nn.GRU(input_size=input_size, hidden_size=hidden_size, batch_first=True)
        self.auxiliary_net = MLPLayers(layers=mlp_size, activation="none")

    def forward(self, keys, keys_length, neg_keys=None):
        rnn_outputs, _ = _gru_padded(self.gru, keys, keys_length)
        aux_loss = self.auxiliary_loss(rnn_outputs[:, :-1, :], keys[:, 1:, :], neg_keys[:, 1:, :], keys_length - 1)
        return rnn_outputs, aux_loss

    def auxiliary_loss(self, h_states, click_seq, noclick_seq, keys_length):
        """The reference's ``binary_cross_entropy_with_logits`` over the rows ``t < keys_length``, written mask-weighted:
        ``(sum m softplus(-click) + sum m softplus(noclick)) / (2 sum m)`` -- no data-dependent shape, no host copy."""
        batch_size, hist_length, _ = h_states.shape
        mask = (torch.arange(hist_length, device=h_states.device).view(1, -1) < keys_length.view(-1, 1)).to(h_states.dtype)
        click_prop = self.auxiliary_net(torch.cat([h_states, click_seq], dim=-1)).view(batch_size, hist_length)
        noclick_prop = self.auxiliary_net(torch.cat([h_states, noclick_seq], dim=-1)).view(batch_size, hist_length)
        total = (mask * F.softplus(-click_prop)).sum() + (mask * F.softplus(noclick_prop)).sum()
        return total / (2 * mask.sum())


class InterestEvolvingLayer(nn.Module):
    """The interest-evolving layer for all four ``gru`` values: 'GRU' (a GRU, then attention pooling of its outputs), 'AIGRU'
    (the scores scale the GRU's inputs), 'AGRU' and 'AUGRU' (the attention-gated recurrence, ``ops.att_gru``).
    ``queries`` [B, E], ``keys`` [B, T, E], ``keys_length`` [B] -> [B, H]; the final state is the op's ``h_n`` (the reference
    gathers the output at position ``keys_length - 1``, the same rows)."""

    def __init__(self, mask_mat, input_size, rnn_hidden_size, att_hidden_size=(80, 40), activation="sigmoid",
                 softmax_stag=True, gru="GRU"):
        super(InterestEvolvingLayer, self).__init__()
        self.mask_mat = mask_mat
        self.gru = gru
        if gru == "GRU":
            self.attention_layer = SequenceAttLayer(mask_mat, att_hidden_size, activation, softmax_stag, False)
            self.dynamic_rnn = nn.GRU(input_size=input_size, hidden_size=rnn_hidden_size, batch_first=True)
        elif gru == "AIGRU":
            self.attention_layer = SequenceAttLayer(mask_mat, att_hidden_size, activation, softmax_stag, True)
            self.dynamic_rnn = nn.GRU(input_size=input_size, hidden_size=rnn_hidden_size, batch_first=True)
        elif gru == "AGRU" or gru == "AUGRU":
            self.attention_layer = SequenceAttLayer(mask_mat, att_hidden_size, activation, softmax_stag, True)
            self.dynamic_rnn = DynamicRNN(input_size=input_size, hidden_size=rnn_hidden_size, gru=gru)

    def final_output(self, outputs, keys_length):
        """The row of ``outputs`` [B, T, H] at position ``keys_length - 1`` (kept for callers; ``forward`` uses ``h_n``)."""
        batch_size, hist_len, _ = outputs.shape
        mask = torch.arange(hist_len, device=keys_length.device).repeat(batch_size, 1) == (keys_length.view(-1, 1) - 1)
        return outputs[mask]

    def forward(self, queries, keys, keys_length):
        if self.gru == "GRU":
            rnn_outputs, _ = _gru_padded(self.dynamic_rnn, keys, keys_length)
            outputs = self.attention_layer(queries, rnn_outputs, keys_length).squeeze(1)
        elif self.gru == "AIGRU":
            att_outputs = self.attention_layer(queries, keys, keys_length)
            interest = keys * att_outputs.transpose(1, 2)
            _, outputs = _gru_padded(self.dynamic_rnn, interest, keys_length)
        elif self.gru == "AGRU" or self.gru == "AUGRU":
            att_outputs = self.attention_layer(queries, keys, keys_length).squeeze(1)          # [B, T]
            _, outputs = self.dynamic_rnn.forward_padded(keys, att_outputs, keys_length)
        return outputs


def _linear(m, x):
    return ops.linear(x, m.weight, m.bias) if x.is_cuda else m(x)


def _lookup(table, ids):
    """table(ids) for an [B, L] id block: the gather kernel on the GPU, nn.Embedding elsewhere."""
    if not ids.is_cuda:
        return table(ids)
    from ..rechub.models.matching import ops_position
    return ops_position(table, ids)


class GNN(nn.Module):
    """``recbole.model.sequential_recommender.srgnn.GNN`` (srgnn.py:29-95; GCSAN carries the same class): same constructor,
    attribute names and ``state_dict`` keys (``w_ih``, ``w_hh``, ``b_ih``, ``b_hh``, ``b_iah``, ``b_ioh``,
    ``linear_edge_in.*``, ``linear_edge_out.*``).  ``forward(A, hidden)`` is ``step`` calls of
    ``ops.session_gnn_step_torch`` (the cell in ATen; it has no fused kernel yet).  The reference leaves the bare parameters
    uninitialised until its model draws them; here they start from the model's own rule, uniform in +- 1 / sqrt(size)."""

    def __init__(self, embedding_size, step=1):
        super(GNN, self).__init__()
        self.step = step
        self.embedding_size = embedding_size
        self.input_size = embedding_size * 2
        self.gate_size = embedding_size * 3
        self.w_ih = nn.Parameter(torch.empty(self.gate_size, self.input_size))
        self.w_hh = nn.Parameter(torch.empty(self.gate_size, self.embedding_size))
        self.b_ih = nn.Parameter(torch.empty(self.gate_size))
        self.b_hh = nn.Parameter(torch.empty(self.gate_size))
        self.b_iah = nn.Parameter(torch.empty(self.embedding_size))
        self.b_ioh = nn.Parameter(torch.empty(self.embedding_size))
        self.linear_edge_in = nn.Linear(self.embedding_size, self.embedding_size, bias=True)
        self.linear_edge_out = nn.Linear(self.embedding_size, self.embedding_size, bias=True)
        stdv = 1.0 / math.sqrt(self.embedding_size)
        for p in (self.w_ih, self.w_hh, self.b_ih, self.b_hh, self.b_iah, self.b_ioh):
            p.data.uniform_(-stdv, stdv)

    def GNNCell(self, A, hidden):
        return ops.session_gnn_step_torch(A, hidden, self.linear_edge_in.weight, self.linear_edge_in.bias, self.linear_edge_out.weight,
                                          self.linear_edge_out.bias, self.b_iah, self.b_ioh, self.w_ih, self.w_hh, self.b_ih, self.b_hh)

    def forward(self, A, hidden):
        for _ in range(self.step):
            hidden = self.GNNCell(A, hidden)
        return hidden


class SRGNNEncoder(nn.Module):
    """The network of ``recbole.model.sequential_recommender.srgnn.SRGNN`` (srgnn.py:126-217) without RecBole's
    ``(config, dataset)`` plumbing: the reference model's ``state_dict`` keys (``item_embedding``, ``gnn``, ``linear_one``,
    ``linear_two``, ``linear_three``, ``linear_transform``) and its ``_reset_parameters``.  ``forward(item_seq, item_seq_len)``
    is srgnn.py:201-217: the session graphs are built on the device (``ops.session_graph_torch``: vectorised ATen, no host copy), the node
    embeddings go through ``GNN``, and the readout -- alpha has no softmax -- runs in ATen.  The last click is looked up at
    ``(item_seq_len - 1).clamp_min(0)``, so an empty session does not fault (the reference's index is -1 there)."""

    def __init__(self, n_items, embedding_size, step=1):
        super(SRGNNEncoder, self).__init__()
        self.n_items = n_items
        self.embedding_size = embedding_size
        self.step = step
        self.item_embedding = nn.Embedding(n_items, embedding_size, padding_idx=0)
        self.gnn = GNN(embedding_size, step)
        self.linear_one = nn.Linear(embedding_size, embedding_size, bias=True)
        self.linear_two = nn.Linear(embedding_size, embedding_size, bias=True)
        self.linear_three = nn.Linear(embedding_size, 1, bias=False)
        self.linear_transform = nn.Linear(embedding_size * 2, embedding_size, bias=True)
        self._reset_parameters()

    def _reset_parameters(self):
        stdv = 1.0 / math.sqrt(self.embedding_size)
        for weight in self.parameters():
            weight.data.uniform_(-stdv, stdv)

    def forward(self, item_seq, item_seq_len):
        alias_inputs, A, items, mask = ops.session_graph_torch(item_seq)
        hidden = self.gnn(A, _lookup(self.item_embedding, items))
        H = self.embedding_size
        seq_hidden = torch.gather(hidden, 1, alias_inputs.unsqueeze(-1).expand(-1, -1, H))
        last = (item_seq_len.long() - 1).clamp_min(0).view(-1, 1, 1).expand(-1, -1, H)
        ht = seq_hidden.gather(1, last).squeeze(1)
        q1 = _linear(self.linear_one, ht).view(ht.size(0), 1, ht.size(1))
        q2 = _linear(self.linear_two, seq_hidden)
        alpha = self.linear_three(torch.sigmoid(q1 + q2))
        a = torch.sum(alpha * seq_hidden * mask.view(mask.size(0), -1, 1).float(), 1)
        return _linear(self.linear_transform, torch.cat([a, ht], dim=1))

    def full_sort_scores(self, item_seq, item_seq_len):
        """[B, n_items]: ``seq_output`` against the whole table (srgnn.py:247-255)."""
        seq_output = self.forward(item_seq, item_seq_len)
        w = self.item_embedding.weight
        return ops.linear(seq_output, w.view_as(w)) if seq_output.is_cuda else torch.matmul(seq_output, w.t())


class CaserEncoder(nn.Module):
    """The network of ``recbole.model.sequential_recommender.caser.Caser`` (caser.py:42-155) without RecBole's ``(config,
    dataset)`` plumbing: the reference model's ``state_dict`` keys (``user_embedding``, ``item_embedding``, ``conv_v``,
    ``conv_h.<h - 1>``, ``fc1``, ``fc2``) and its ``_init_weights``.  ``conv_v`` and ``conv_h`` are ``nn.Conv2d`` modules kept as
    parameter holders: ``forward(user, item_seq)`` is caser.py:114-145 with both convolution branches, the ReLU, the max over
    time and the two concatenations as one ``ops.caser_conv`` call, the dropout as ``ops.dropout`` and the two fully-connected
    layers as ``ops.linear(..., act="relu")``.  As in the reference, ``max_seq_length`` fixes L and padded positions are zero
    rows that are convolved like the others."""

    def __init__(self, n_users, n_items, embedding_size, max_seq_length, n_h, n_v, dropout_prob=0.0, reg_weight=0.0):
        super(CaserEncoder, self).__init__()
        self.n_users, self.n_items = n_users, n_items
        self.embedding_size = embedding_size
        self.max_seq_length = max_seq_length
        self.n_h, self.n_v = n_h, n_v
        self.dropout_prob = dropout_prob
        self.reg_weight = reg_weight
        self.user_embedding = nn.Embedding(n_users, embedding_size, padding_idx=0)
        self.item_embedding = nn.Embedding(n_items, embedding_size, padding_idx=0)
        self.conv_v = nn.Conv2d(in_channels=1, out_channels=n_v, kernel_size=(max_seq_length, 1))
        self.conv_h = nn.ModuleList([nn.Conv2d(in_channels=1, out_channels=n_h, kernel_size=(i + 1, embedding_size))
                                     for i in range(max_seq_length)])
        self.fc1_dim_v = n_v * embedding_size
        self.fc1_dim_h = n_h * max_seq_length
        self.fc1 = nn.Linear(self.fc1_dim_v + self.fc1_dim_h, embedding_size)
        self.fc2 = nn.Linear(embedding_size + embedding_size, embedding_size)
        self.apply(self._init_weights)

    def _init_weights(self, module):
        if isinstance(module, nn.Embedding):
            nn.init.normal_(module.weight.data, 0, 1.0 / module.embedding_dim)
        elif isinstance(module, nn.Linear):
            nn.init.xavier_normal_(module.weight.data)
            if module.bias is not None:
                nn.init.constant_(module.bias.data, 0)

    def conv(self, item_seq_emb):
        """[B, n_v D + n_h L] of an embedded session [B, L, D]: caser.py:121-137."""
        w_h = [c.weight for c in self.conv_h] if self.n_h else []
        b_h = [c.bias for c in self.conv_h] if self.n_h else []
        return ops.caser_conv(item_seq_emb, self.conv_v.weight if self.n_v else None, self.conv_v.bias if self.n_v else None,
                              w_h, b_h)

    def forward(self, user, item_seq):
        item_seq_emb = _lookup(self.item_embedding, item_seq)                                # [B, L, D]
        user_emb = _lookup(self.user_embedding, user.reshape(-1, 1)).squeeze(1)             # [B, D]
        out = self.conv(item_seq_emb)
        if out.is_cuda:
            out = ops.dropout(out, self.dropout_prob, self.training)
            z = ops.linear(out, self.fc1.weight, self.fc1.bias, act="relu")
            return ops.linear(torch.cat([z, user_emb], 1), self.fc2.weight, self.fc2.bias, act="relu")
        out = F.dropout(out, self.dropout_prob, self.training)
        z = F.relu(self.fc1(out))
        return F.relu(self.fc2(torch.cat([z, user_emb], 1)))

    def reg_loss_conv_h(self):
        """L2 loss on conv_h (caser.py:147-155): ``reg_weight`` times the sum of the filters' 2-norms."""
        loss_conv_h = 0
        for name, parm in self.conv_h.named_parameters():
            if name.endswith("weight"):
                loss_conv_h = loss_conv_h + parm.norm(2)
        return self.reg_weight * loss_conv_h

    def full_sort_scores(self, user, item_seq):
        """[B, n_items]: ``seq_output`` against the whole table (caser.py:196-204)."""
        seq_output = self.forward(user, item_seq)
        w = self.item_embedding.weight
        return ops.linear(seq_output, w.view_as(w)) if seq_output.is_cuda else torch.matmul(seq_output, w.t())
