"""Generate tests/golden/srgnn.npz from the LIVE reference (dev container only; run from the repository root):

    python tests/gen_golden_srgnn.py

RecBole's SR-GNN (third_party/recbole/model/sequential_recommender/srgnn.py): the reference's ``GNN`` itself, and
``SRGNN._get_slice`` / ``SRGNN.forward`` called unbound on a stand-in module that carries what they read --
``embedding_size``, ``device``, ``item_embedding`` (``nn.Embedding(padding_idx=0)``), ``gnn``, ``linear_one``, ``linear_two``,
``linear_three``, ``linear_transform``, ``gather_indexes`` -- because the model's constructor wants RecBole's config and
dataset.  The parameters are drawn by the reference's ``_reset_parameters`` under a seed.

Groups.  ``graph``: hand-written sessions ``seq`` [12, 10] -- an empty row, a full row without 0, a single click, one item
repeated, a repeated transition, an id above 2^31, a 0 in the first position, a self-loop -- with the ``alias``, ``A`` and
``items`` of ``_get_slice``.  Per model case c at (B, L, H, step, n_items) = (37, 10, 16, 1, 23), (19, 7, 8, 2, 11) and
(11, 5, 4, 2, 6): ``in<c>`` (``seq`` left-aligned sessions of 1 .. L clicks with dense repeats, ``len``, ``up`` [B, H]),
``p<c>`` (the stand-in's state_dict, whose keys are the reference model's), ``out<c>`` (``alias``, ``A``, ``items`` and
``seq_output`` = forward(seq, len) [B, H]) and ``g<c>`` (the gradients of ``sum(seq_output * up)`` with respect to every
parameter).  The model cases hold no empty session: the reference's last-click gather faults there.  Data only.

The reference package imports its vendored deepctr, which asks a package index for its latest version from a thread when
imported; generation runs offline, so stand-ins for ``requests`` (whose ``get`` raises) and for that package are registered
before the reference is imported and no request is ever started (as in tests/gen_golden_fignn.py)."""
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = ((37, 10, 16, 1, 23), (19, 7, 8, 2, 11), (11, 5, 4, 2, 6))
BIG = (1 << 31) + 5
GRAPH_SESSIONS = [
    [0, 0, 0, 0, 0, 0, 0, 0, 0, 0],                  # empty
    [9, 3, 7, 1, 8, 2, 6, 4, 10, 5],                 # full, no 0, all distinct
    [4, 0, 0, 0, 0, 0, 0, 0, 0, 0],                  # a single click
    [6, 6, 6, 6, 6, 0, 0, 0, 0, 0],                  # one item repeated (a self-loop, set once)
    [2, 5, 2, 5, 2, 5, 3, 0, 0, 0],                  # repeated transitions 2 -> 5 and 5 -> 2
    [BIG, 3, BIG + 1, 3, BIG, 0, 0, 0, 0, 0],        # ids above 2^31
    [0, 7, 8, 0, 9, 9, 0, 0, 0, 0],                  # a 0 in front is a node with an edge; nothing after the next 0
    [1, 2, 3, 2, 4, 2, 1, 2, 3, 3],                  # full with repeats: in- and out-degrees up to 3
    [5, 4, 3, 2, 1, 0, 1, 2, 3, 4],                  # clicks behind a 0 give nodes but no edges
    [3, 3, 0, 0, 0, 0, 0, 0, 0, 0],
    [7, 1, 7, 1, 7, 1, 7, 1, 7, 1],
    [10, 9, 8, 7, 6, 5, 4, 3, 2, 0],
]


def _stand_in(mod, n_items, H, step):
    nn = torch.nn
    host = nn.Module()
    host.embedding_size, host.step, host.device = H, step, torch.device("cpu")
    host.item_embedding = nn.Embedding(n_items, H, padding_idx=0)
    host.gnn = mod.GNN(H, step)
    host.linear_one = nn.Linear(H, H, bias=True)
    host.linear_two = nn.Linear(H, H, bias=True)
    host.linear_three = nn.Linear(H, 1, bias=False)
    host.linear_transform = nn.Linear(H * 2, H, bias=True)
    host._get_slice = lambda item_seq: mod.SRGNN._get_slice(host, item_seq)
    host.gather_indexes = lambda output, index: output.gather(
        1, index.view(-1, 1, 1).expand(-1, -1, output.shape[-1])).squeeze(1)      # SequentialRecommender.gather_indexes
    mod.SRGNN._reset_parameters(host)
    return host


def _sessions(B, L, n_items, g):
    lengths = torch.randint(1, L + 1, (B,), generator=g)
    lengths[0], lengths[1] = L, 1                                                   # a full row and a single click
    seq = torch.randint(1, n_items, (B, L), generator=g)
    seq = seq * (torch.arange(L).unsqueeze(0) < lengths.unsqueeze(1))
    if L >= 5:
        seq[2, :5] = torch.tensor([3, 3, 3, 3, 3])                                  # one item repeated
        seq[3, :5] = torch.tensor([1, 2, 1, 2, 4])                                  # a repeated transition
        seq[2, 5:], seq[3, 5:] = 0, 0
        lengths[2], lengths[3] = 5, 5
    return seq, lengths


def record(c, dims, mod, out):
    B, L, H, step, n_items = dims
    torch.manual_seed(900 + c)
    g = torch.Generator().manual_seed(400 + c)
    host = _stand_in(mod, n_items, H, step)
    seq, lengths = _sessions(B, L, n_items, g)
    up = torch.randn(B, H, generator=g)
    alias, A, items, _ = mod.SRGNN._get_slice(host, seq)
    y = mod.SRGNN.forward(host, seq, lengths)
    assert tuple(y.shape) == (B, H)
    (y * up).sum().backward()
    out.update({"in%d.seq" % c: seq.numpy(), "in%d.len" % c: lengths.numpy(), "in%d.up" % c: up.numpy(),
                "out%d.alias" % c: alias.numpy(), "out%d.A" % c: A.numpy(), "out%d.items" % c: items.numpy(),
                "out%d.seq_output" % c: y.detach().numpy()})
    params = dict(host.named_parameters())
    assert sorted(params) == sorted(host.state_dict())
    for k, v in params.items():
        out["p%d.%s" % (c, k)] = v.detach().numpy()
        out["g%d.%s" % (c, k)] = v.grad.numpy()
    print("case %d %s: |seq_output| max %.3f" % (c, dims, float(y.detach().abs().max())))


def main():
    import gen_golden_autoint
    gen_golden_autoint._offline()
    import gen_golden_recbole
    gen_golden_recbole.recbole_layers()
    mod = importlib.import_module("recbox.third_party.recbole.model.sequential_recommender.srgnn")
    out = {}
    seq = torch.tensor(GRAPH_SESSIONS, dtype=torch.int64)
    host = _stand_in(mod, 4, 4, 1)
    alias, A, items, mask = mod.SRGNN._get_slice(host, seq)
    assert A.dtype == torch.float32 and alias.dtype == torch.int64 and items.dtype == torch.int64
    out.update({"graph.seq": seq.numpy(), "graph.alias": alias.numpy(), "graph.A": A.numpy(), "graph.items": items.numpy()})
    for c, dims in enumerate(CASES):
        record(c, dims, mod, out)
    path = os.path.join(ROOT, "tests", "golden", "srgnn.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d arrays, %d bytes)" % (path, len(out), os.path.getsize(path)))
    assert os.path.getsize(path) < 512 * 1024


if __name__ == "__main__":
    main()
