"""The attention-gated GRU layer of DIEN restated in plain torch ops (run in float64 and in float32 by the tests): the
reference cells' gate convention (third_party/recbole/model/sequential_recommender/dien.py:389-475), ``lengths`` with
packed-sequence semantics, ``h0``, both cells.

    rows of w_ih [3H, I] and w_hh [3H, H]: r, u, n          a = att[b, t]
    gi = x w_ih^T + b_ih        gh = h w_hh^T + b_hh
    r = s(gi_r + gh_r)   u = s(gi_u + gh_u)   n = tanh(gi_n + r gh_n)
    AUGRU: c = a u        AGRU: c = a  (u is not formed: the u rows of the parameters get zero gradients)
    h' = (1 - c) h + c n
    t >= lengths[b]: the state is frozen and the output at that position is 0; h_n[b] is the state after step lengths[b] - 1
    (lengths[b] = 0: h_n[b] = h0[b] and an all-zero row)."""
import torch


def cell_step(cell, x, h, a, w_ih, w_hh, b_ih=None, b_hh=None):
    """One step: x [B, I], h [B, H], a [B] -> h' [B, H]."""
    H = w_hh.shape[1]
    gi = x @ w_ih.t()
    if b_ih is not None:
        gi = gi + b_ih
    gh = h @ w_hh.t()
    if b_hh is not None:
        gh = gh + b_hh
    r = torch.sigmoid(gi[:, :H] + gh[:, :H])
    n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
    c = a.reshape(-1, 1)
    if cell == "AUGRU":
        c = c * torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
    elif cell != "AGRU":
        raise ValueError(cell)
    return (1 - c) * h + c * n


def att_gru_layer(x, att, w_ih, w_hh, b_ih=None, b_hh=None, h0=None, lengths=None, cell="AUGRU"):
    """x [B, L, I], att [B, L] -> (out [B, L, H], h_n [B, H])."""
    B, L, _ = x.shape
    H = w_hh.shape[1]
    h = h0 if h0 is not None else x.new_zeros(B, H)
    outs = []
    for t in range(L):
        new = cell_step(cell, x[:, t], h, att[:, t], w_ih, w_hh, b_ih, b_hh)
        if lengths is not None:
            act = (lengths > t).unsqueeze(1)
            h = torch.where(act, new, h)
            outs.append(torch.where(act, new, torch.zeros_like(new)))
        else:
            h = new
            outs.append(new)
    return torch.stack(outs, dim=1), h
