"""Generate tests/golden/fignn.npz from the LIVE reference (dev container only; run from the repository root):

    python tests/gen_golden_fignn.py

RecBole's ``FiGNN.fignn_layer`` (third_party/recbole/model/context_aware_recommender/fignn.py:107-144), called unbound on a
stand-in module that carries what it reads -- ``att_embedding``, ``self_attn`` (a real ``nn.MultiheadAttention(batch_first=
True)``), ``v_res_embedding``, ``gnn`` (the reference's ``GraphLayer``s), ``W_attn``, ``gru_cell`` (a real ``nn.GRUCell``),
``mlp1``, ``mlp2``, ``dropout_layer``, ``leaky_relu``, ``src_nodes``, ``dst_nodes``, ``num_feature_field``,
``attention_size``, ``n_layers``, ``device`` -- because the model's constructor wants RecBole's config and dataset.  Every
dropout is 0.  Seeded Gaussian inputs on the CPU at (B, F, D, A, heads, n_layers) = (37, 5, 8, 16, 2, 3), (19, 7, 16, 32, 4, 2)
and (11, 3, 4, 8, 1, 1).  Groups per case c: ``in<c>`` (``x`` [B, F, D], ``up`` [B, 1]), ``p<c>`` (the stand-in's state_dict,
whose keys are the reference model's), ``out<c>`` (``y`` = fignn_layer(x) [B, 1] and ``graph`` [B, F, F]) and ``g<c>`` (the
gradients of ``sum(y * up)`` with respect to ``x`` and every parameter that has one).  A seed is refused when a pre-relu value
of the first stage or an off-diagonal leaky-relu argument lies within 1e-4 of zero, so that fp32 rounding on another device
cannot flip a unit or a slope.  Data only.

The reference package imports its vendored deepctr, which asks a package index for its latest version from a thread when
imported; generation runs offline, so stand-ins for ``requests`` (whose ``get`` raises) and for that package are registered
before the reference is imported and no request is ever started (as in tests/gen_golden_autoint.py)."""
import importlib
import os
import sys
from itertools import product

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = ((37, 5, 8, 16, 2, 3), (19, 7, 16, 32, 4, 2), (11, 3, 4, 8, 1, 1))
MIN_MARGIN = 1e-4


def _host(dims, mod, g):
    """What ``FiGNN.fignn_layer`` reads of its model, every parameter a seeded Gaussian."""
    B, F, D, A, h, n_layers = dims
    nn = torch.nn
    host = nn.Module()
    host.dropout_layer = nn.Dropout(p=0.0)
    host.att_embedding = nn.Linear(D, A)
    host.self_attn = nn.MultiheadAttention(A, h, dropout=0.0, batch_first=True)
    host.v_res_embedding = nn.Linear(D, A)
    host.src_nodes, host.dst_nodes = zip(*list(product(range(F), repeat=2)))
    host.gnn = nn.ModuleList([mod.GraphLayer(F, A) for _ in range(n_layers - 1)])
    host.leaky_relu = nn.LeakyReLU(negative_slope=0.01)
    host.W_attn = nn.Linear(A * 2, 1, bias=False)
    host.gru_cell = nn.GRUCell(A, A)
    host.mlp1 = nn.Linear(A, 1, bias=False)
    host.mlp2 = nn.Linear(F * A, F, bias=False)
    host.num_feature_field, host.attention_size, host.n_layers, host.device = F, A, n_layers, torch.device("cpu")
    with torch.no_grad():
        for name, p in host.named_parameters():
            fan_in = p.shape[-1] if p.dim() > 1 else 4
            p.copy_(torch.randn(p.shape, generator=g) * (1.0 / fan_in ** 0.5))
    return host


def _margin(host, x):
    """The smallest |pre-relu value| of the first stage and |off-diagonal leaky-relu argument| of the graph."""
    F = host.num_feature_field
    with torch.no_grad():
        emb = host.att_embedding(x)
        att, _ = host.self_attn(emb, emb, emb)
        pre = att + host.v_res_embedding(x)
        att = torch.relu(pre)
        cat = torch.cat([att[:, host.src_nodes, :], att[:, host.dst_nodes, :]], dim=-1)
        arg = host.W_attn(cat).view(-1, F, F).abs().masked_fill(torch.eye(F, dtype=torch.bool), float("inf"))
    return float(min(pre.abs().min(), arg.min()))


def record(c, dims, mod, out):
    B, F, D = dims[:3]
    for seed in range(200 + c, 600, 3):
        g = torch.Generator().manual_seed(seed)
        host = _host(dims, mod, g)
        x = torch.randn(B, F, D, generator=g).requires_grad_()
        up = torch.randn(B, 1, generator=g)
        closest = _margin(host, x.detach())
        if closest > MIN_MARGIN:
            break
    else:
        raise RuntimeError("no seed keeps every margin for %s" % (dims,))
    y = mod.FiGNN.fignn_layer(host, x)
    assert tuple(y.shape) == (B, 1)
    (y * up).sum().backward()
    print("case %d %s: seed %d, smallest margin %.2e" % (c, dims, seed, closest))
    out.update({"in%d.x" % c: x.detach().numpy(), "in%d.up" % c: up.numpy(), "out%d.y" % c: y.detach().numpy(),
                "out%d.graph" % c: host.graph.detach().numpy(), "g%d.x" % c: x.grad.numpy()})
    params = dict(host.named_parameters())
    assert sorted(params) == sorted(host.state_dict())
    for k, v in params.items():
        out["p%d.%s" % (c, k)] = v.detach().numpy()
        if v.grad is not None:
            out["g%d.%s" % (c, k)] = v.grad.numpy()
        else:
            print("  no gradient: %s" % k)


def main():
    import gen_golden_autoint
    gen_golden_autoint._offline()
    import gen_golden_recbole
    gen_golden_recbole.recbole_layers()
    mod = importlib.import_module("recbox.third_party.recbole.model.context_aware_recommender.fignn")
    out = {}
    for c, dims in enumerate(CASES):
        record(c, dims, mod, out)
    path = os.path.join(ROOT, "tests", "golden", "fignn.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d arrays, %d bytes)" % (path, len(out), os.path.getsize(path)))
    assert os.path.getsize(path) < 512 * 1024


if __name__ == "__main__":
    main()
