"""Generate tests/golden/dien.npz from the LIVE reference (dev container only; run from the repository root):

    python tests/gen_golden_dien.py

RecBole's DIEN layers (third_party/recbole/model/sequential_recommender/dien.py:193-521 with ``MLPLayers`` and
``SequenceAttLayer`` of model/layers.py) on the CPU at (B, L, E) = (19, 7, 8) and (11, 5, 12), ``att_hidden_size`` [4E, 16, 8]:
``AGRUCell`` and ``AUGRUCell`` (one step each), ``DynamicRNN`` on packed inputs (both cells), ``InterestEvolvingLayer`` for
'GRU', 'AIGRU', 'AGRU', 'AUGRU' and ``InterestExtractorNetwork`` with negatives.  The lengths are drawn in 1 .. L with at least
one 1 and one L (the reference's packing refuses 0).  Groups per case c = 0, 1: ``in<c>`` (``keys``, ``neg`` [B, L, E],
``queries``, ``h``, ``up_vec`` [B, E], ``att`` [B, L], ``a`` [B], ``lengths`` [B], ``up_seq`` [B, L, E]) and, per module tag
(``agru``, ``augru``, ``dyn_agru``, ``dyn_augru``, ``evo_GRU``, ``evo_AIGRU``, ``evo_AGRU``, ``evo_AUGRU``, ``ext``),
``p<c>_<tag>`` (the state_dict), ``out<c>_<tag>`` and ``g<c>_<tag>`` (the gradients of ``sum(out * up) + aux`` with respect to
the inputs and every parameter).  ``DynamicRNN``'s packed output is recorded padded ([B, L, E], zeros beyond the lengths).
The cells' ``torch.randn`` weights are scaled by 0.3 and their biases drawn, so that the gates do not saturate.  Data only:
274 KB of float32 values (most of it the state_dicts and parameter gradients of the nine modules per case), about 310 KB
on disk.

The reference package imports its vendored deepctr, which asks a package index for its latest version from a thread when
imported; generation runs offline, so stand-ins for ``requests`` (whose ``get`` raises) and for that package are registered
before the reference is imported and no request is ever started."""
import importlib
import os
import sys
import types

import numpy as np
import torch
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

CASES = ((19, 7, 8), (11, 5, 12))


def _offline():
    def refuse(*a, **k):
        raise OSError("offline")
    req = types.ModuleType("requests")
    req.get = refuse
    sys.modules["requests"] = req
    sys.modules["recbox.third_party.deepctr"] = types.ModuleType("recbox.third_party.deepctr")


def _put(out, c, tag, module, outputs, grads):
    for k, v in module.state_dict().items():
        out["p%d_%s.%s" % (c, tag, k)] = v.detach().numpy().copy()
    for k, v in outputs.items():
        out["out%d_%s.%s" % (c, tag, k)] = v.detach().numpy().copy()
    for k, v in grads.items():
        out["g%d_%s.%s" % (c, tag, k)] = v.grad.numpy().copy()
    for k, p in module.named_parameters():
        out["g%d_%s.%s" % (c, tag, k)] = (p.grad if p.grad is not None else torch.zeros_like(p)).numpy().copy()


def _tame_cell(cell, g):
    with torch.no_grad():
        cell.weight_ih.mul_(0.3)
        cell.weight_hh.mul_(0.3)
        cell.bias_ih.copy_(torch.randn(cell.bias_ih.shape, generator=g) * 0.1)
        cell.bias_hh.copy_(torch.randn(cell.bias_hh.shape, generator=g) * 0.1)


def record(c, dims, D, out):
    B, L, E = dims
    g = torch.Generator().manual_seed(500 + c)
    torch.manual_seed(700 + c)
    lengths = torch.randint(1, L + 1, (B,), generator=g)
    lengths[0], lengths[1] = 1, L
    t = {"keys": torch.randn(B, L, E, generator=g), "neg": torch.randn(B, L, E, generator=g),
         "queries": torch.randn(B, E, generator=g), "h": torch.randn(B, E, generator=g) * 0.5,
         "att": torch.rand(B, L, generator=g), "a": torch.rand(B, generator=g),
         "up_seq": torch.randn(B, L, E, generator=g), "up_vec": torch.randn(B, E, generator=g)}
    for k, v in t.items():
        out["in%d.%s" % (c, k)] = v.numpy().copy()
    out["in%d.lengths" % c] = lengths.numpy().copy()

    def leaf(name):
        return t[name].clone().requires_grad_()

    for tag, cls in (("agru", D.AGRUCell), ("augru", D.AUGRUCell)):
        cell = cls(E, E)
        _tame_cell(cell, g)
        x, h, a = t["keys"][:, 0].clone().requires_grad_(), leaf("h"), leaf("a")
        hy = cell(x, h, a)
        (hy * t["up_vec"]).sum().backward()
        _put(out, c, tag, cell, {"hy": hy}, {"x": x, "h": h, "a": a})

    for tag, kind in (("dyn_agru", "AGRU"), ("dyn_augru", "AUGRU")):
        rnn = D.DynamicRNN(E, E, gru=kind)
        _tame_cell(rnn.rnn, g)
        keys, att = leaf("keys"), leaf("att")
        pk = pack_padded_sequence(keys, lengths=lengths, batch_first=True, enforce_sorted=False)
        pa = pack_padded_sequence(att, lengths=lengths, batch_first=True, enforce_sorted=False)
        y, _ = pad_packed_sequence(rnn(pk, pa), batch_first=True, padding_value=0.0, total_length=L)
        (y * t["up_seq"]).sum().backward()
        _put(out, c, tag, rnn, {"out": y}, {"keys": keys, "att": att})

    mask_mat = torch.arange(L).view(1, -1)
    for kind in ("GRU", "AIGRU", "AGRU", "AUGRU"):
        layer = D.InterestEvolvingLayer(mask_mat, E, E, [4 * E, 16, 8], gru=kind)
        if kind in ("AGRU", "AUGRU"):
            _tame_cell(layer.dynamic_rnn.rnn, g)
        queries, keys = leaf("queries"), leaf("keys")
        y = layer(queries, keys, lengths)
        assert tuple(y.shape) == (B, E)
        (y * t["up_vec"]).sum().backward()
        _put(out, c, "evo_" + kind, layer, {"y": y}, {"queries": queries, "keys": keys})

    ext = D.InterestExtractorNetwork(E, E, [2 * E, 16, 1])
    keys, neg = leaf("keys"), leaf("neg")
    rnn_out, aux = ext(keys, lengths, neg)
    ((rnn_out * t["up_seq"]).sum() + aux).backward()
    _put(out, c, "ext", ext, {"rnn": rnn_out, "aux": aux}, {"keys": keys, "neg": neg})
    print("case %d %s: lengths %s" % (c, dims, lengths.tolist()))


def main():
    _offline()
    import gen_golden_recbole
    gen_golden_recbole.recbole_layers()
    D = importlib.import_module("recbox.third_party.recbole.model.sequential_recommender.dien")
    out = {}
    for c, dims in enumerate(CASES):
        record(c, dims, D, out)
    path = os.path.join(ROOT, "tests", "golden", "dien.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d arrays, %d bytes)" % (path, len(out), os.path.getsize(path)))
    assert os.path.getsize(path) < 512 * 1024


if __name__ == "__main__":
    main()
