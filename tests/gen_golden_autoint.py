"""Generate tests/golden/autoint.npz from the LIVE reference (dev container only; run from the repository root):

    python tests/gen_golden_autoint.py

RecBole's ``AutoInt.autoint_layer`` (third_party/recbole/model/context_aware_recommender/autoint.py:78-103), called unbound on
a stand-in module that carries what it reads -- ``att_embedding``, ``self_attns`` (real ``nn.MultiheadAttention``),
``mlp_layers`` (the reference's ``MLPLayers``), ``attn_fc``, ``deep_predict_layer``, ``v_res_embedding``, ``has_residual``,
``atten_output_dim`` -- because the model's constructor wants RecBole's config and dataset.  Every dropout is 0.  Seeded
Gaussian inputs on the CPU at (B, F, D, A, heads, layers, residual) = (37, 5, 8, 16, 2, 3, True) and (19, 7, 16, 32, 4, 2,
False), MLP sizes (32, 16).  Groups per case c = 0, 1: ``in<c>`` (``x`` [B, F, D], ``up`` [B, 1]), ``p<c>`` (the stand-in's
state_dict, whose keys are the reference model's), ``out<c>`` (``y`` = autoint_layer(x) [B, 1] and ``att<i>`` [B, heads, F, F],
the per-head probabilities of layer i) and ``g<c>`` (the gradients of ``sum(y * up)`` with respect to ``x`` and every
parameter).  A seed is refused when a pre-relu value -- of the final relu or of the MLP's -- lies within 1e-4 of zero, so that
fp32 rounding on another device cannot flip a unit.  Data only.

The reference package imports its vendored deepctr, which asks a package index for its latest version from a thread when
imported; generation runs offline, so stand-ins for ``requests`` (whose ``get`` raises) and for that package are registered
before the reference is imported and no request is ever started."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

CASES = ((37, 5, 8, 16, 2, 3, True), (19, 7, 16, 32, 4, 2, False))
MLP = [32, 16]
MIN_PRE_RELU = 1e-4


def _offline():
    def refuse(*a, **k):
        raise OSError("offline")
    req = types.ModuleType("requests")
    req.get = refuse
    sys.modules["requests"] = req
    sys.modules["recbox.third_party.deepctr"] = types.ModuleType("recbox.third_party.deepctr")


def _host(dims, L, g):
    """What ``AutoInt.autoint_layer`` reads of its model, every parameter a seeded Gaussian."""
    B, F, D, A, h, n_layers, residual = dims
    host = torch.nn.Module()
    host.att_embedding = torch.nn.Linear(D, A)
    host.mlp_layers = L.MLPLayers([F * D] + MLP, dropout=0.0)
    host.self_attns = torch.nn.ModuleList([torch.nn.MultiheadAttention(A, h, dropout=0.0) for _ in range(n_layers)])
    host.attn_fc = torch.nn.Linear(F * A, 1)
    host.deep_predict_layer = torch.nn.Linear(MLP[-1], 1)
    if residual:
        host.v_res_embedding = torch.nn.Linear(D, A)
    host.has_residual = residual
    host.atten_output_dim = F * A
    with torch.no_grad():
        for name, p in host.named_parameters():
            fan_in = p.shape[-1] if p.dim() > 1 else 4
            p.copy_(torch.randn(p.shape, generator=g) * (1.0 / fan_in ** 0.5))
    return host


def _pre_relu(host, x):
    """The smallest |pre-relu value| of the final relu and of the MLP's, and the per-head probabilities of every layer."""
    vals, atts = [], []
    with torch.no_grad():
        cross = host.att_embedding(x).transpose(0, 1)
        for attn in host.self_attns:
            cross, w = attn(cross, cross, cross, need_weights=True, average_attn_weights=False)
            atts.append(w)
        cross = cross.transpose(0, 1)
        if host.has_residual:
            cross = cross + host.v_res_embedding(x)
        vals.append(cross.abs().min())
        z = x.reshape(x.shape[0], -1)
        for m in host.mlp_layers.mlp_layers:
            z = m(z)
            if isinstance(m, torch.nn.Linear):
                vals.append(z.abs().min())
    return float(min(vals)), atts


def record(c, dims, L, AutoInt, out):
    B, F, D = dims[:3]
    for seed in range(100 + c, 300, 2):
        g = torch.Generator().manual_seed(seed)
        host = _host(dims, L, g)
        x = torch.randn(B, F, D, generator=g).requires_grad_()
        up = torch.randn(B, 1, generator=g)
        closest, atts = _pre_relu(host, x.detach())
        if closest > MIN_PRE_RELU:
            break
    else:
        raise RuntimeError("no seed keeps every pre-relu value away from zero for %s" % (dims,))
    y = AutoInt.autoint_layer(host, x)
    assert tuple(y.shape) == (B, 1)
    (y * up).sum().backward()
    print("case %d %s: seed %d, smallest |pre-relu| %.2e" % (c, dims, seed, closest))
    out.update({"in%d.x" % c: x.detach().numpy(), "in%d.up" % c: up.numpy(), "out%d.y" % c: y.detach().numpy(),
                "g%d.x" % c: x.grad.numpy()})
    for i, a in enumerate(atts):
        out["out%d.att%d" % (c, i)] = a.numpy()
    params = dict(host.named_parameters())
    assert sorted(params) == sorted(host.state_dict())
    for k, v in params.items():
        out["p%d.%s" % (c, k)] = v.detach().numpy()
        out["g%d.%s" % (c, k)] = v.grad.numpy()


def main():
    _offline()
    import gen_golden_recbole
    L = gen_golden_recbole.recbole_layers()
    import importlib
    AutoInt = importlib.import_module("recbox.third_party.recbole.model.context_aware_recommender.autoint").AutoInt
    out = {}
    for c, dims in enumerate(CASES):
        record(c, dims, L, AutoInt, out)
    path = os.path.join(ROOT, "tests", "golden", "autoint.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d arrays, %d bytes)" % (path, len(out), os.path.getsize(path)))
    assert os.path.getsize(path) < 512 * 1024


if __name__ == "__main__":
    main()
