"""The GRU layer restated in plain torch ops (run in float64 by the tests): torch's gate convention, ``lengths`` with
packed-sequence semantics, ``h0``, stacked layers; and, on top of it, the user tower of GRU4Rec and the score matrix of NARM
as the reference writes them (third_party/rechub/models/matching/gru4rec.py:60-75, narm.py:44-76).

    rows of w_ih [3H, I] and w_hh [3H, H]: r, z, n
    gi = x w_ih^T + b_ih        gh = h w_hh^T + b_hh
    r = s(gi_r + gh_r)   z = s(gi_z + gh_z)   n = tanh(gi_n + r gh_n)   h' = (1 - z) n + z h
    t >= lengths[b]: the state is frozen and the output at that position is 0; h_n[b] is the state after step lengths[b] - 1
    (lengths[b] = 0: h_n[b] = h0[b] and an all-zero row)."""
import torch


def gru_layer(x, w_ih, w_hh, b_ih=None, b_hh=None, h0=None, lengths=None):
    """x [B, L, I] -> (out [B, L, H], h_n [B, H])."""
    B, L, _ = x.shape
    H = w_hh.shape[1]
    h = h0 if h0 is not None else x.new_zeros(B, H)
    gi = x @ w_ih.t()
    if b_ih is not None:
        gi = gi + b_ih
    outs = []
    for t in range(L):
        gh = h @ w_hh.t()
        if b_hh is not None:
            gh = gh + b_hh
        g = gi[:, t]
        r = torch.sigmoid(g[:, :H] + gh[:, :H])
        z = torch.sigmoid(g[:, H:2 * H] + gh[:, H:2 * H])
        n = torch.tanh(g[:, 2 * H:] + r * gh[:, 2 * H:])
        new = (1 - z) * n + z * h
        if lengths is not None:
            act = (lengths > t).unsqueeze(1)
            h = torch.where(act, new, h)
            outs.append(torch.where(act, new, torch.zeros_like(new)))
        else:
            h = new
            outs.append(new)
    return torch.stack(outs, dim=1), h


def gru(x, layers, h0=None, lengths=None):
    """Stacked layers: ``layers`` = [(w_ih, w_hh, b_ih or None, b_hh or None)], h0 [num_layers, B, H] or None
    -> (out [B, L, H], h_n [num_layers, B, H])."""
    finals = []
    for k, (w_ih, w_hh, b_ih, b_hh) in enumerate(layers):
        x, h = gru_layer(x, w_ih, w_hh, b_ih, b_hh, h0[k] if h0 is not None else None, lengths)
        finals.append(h)
    return x, torch.stack(finals, dim=0)


def layers_of(sd, prefix, num_layers, bias):
    """The parameters of a torch-named GRU out of a state_dict."""
    return [(sd["%sweight_ih_l%d" % (prefix, k)], sd["%sweight_hh_l%d" % (prefix, k)],
             sd["%sbias_ih_l%d" % (prefix, k)] if bias else None, sd["%sbias_hh_l%d" % (prefix, k)] if bias else None)
            for k in range(num_layers)]


def narm_scores(sd, ids):
    """NARM's score matrix [B, V] (narm.py:44-76, dropout 0) from its state_dict and the left-aligned session ids [B, L]."""
    mask = ids != 0
    h, h_n = gru(sd["item_emb.weight"][ids], layers_of(sd, "gru.", 1, True), lengths=mask.sum(dim=1))
    h_t = h_n[0]
    q = torch.sigmoid((h_t @ sd["a_1"].t()).unsqueeze(1) + h @ sd["a_2"].t()) @ sd["v"]
    alpha = torch.exp(q) * mask.unsqueeze(-1)
    alpha = alpha / alpha.sum(dim=1, keepdim=True)
    c = torch.cat((h_t, (alpha * h).sum(1)), dim=1)
    return c @ sd["b"].t() @ sd["item_emb.weight"].t()


def gru4rec_history_state(sd, hist, num_layers):
    """The last layer's final state [B, D] of GRU4Rec's bias-free GRU over the embedded history (gru4rec.py:65-67)."""
    x = sd["embedding.embed_dict.item_id.weight"][hist]
    return gru(x, layers_of(sd, "gru.", num_layers, False))[1][-1]
