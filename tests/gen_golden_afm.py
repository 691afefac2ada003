"""Generate tests/golden/afm.npz from the LIVE reference (dev container only; run from the repository root):

    python tests/gen_golden_afm.py

RecBole's ``AttLayer`` (third_party/recbole/model/layers.py) and ``AFM.afm_layer`` (model/context_aware_recommender/afm.py),
the latter called unbound on a small stand-in object that carries what it reads -- ``num_feature_field``, ``attlayer``, ``p``,
``dropout_layer`` (p = 0) and ``build_cross`` -- because the model's constructor wants RecBole's config and dataset.  Seeded
Gaussian inputs on the CPU at (B, F, D, A) = (37, 5, 8, 25) and (19, 7, 16, 32).  Groups per case c = 0, 1: ``in<c>`` (``x``
[B, F, D], ``up`` [B, 1], ``z`` [B, 6, D]), ``p<c>`` (the state_dict: ``attlayer.w.weight``, ``attlayer.h``, ``p``),
``out<c>`` (``y`` = afm_layer(x) [B, 1], ``att`` = AttLayer on the pair products [B, P], ``att_z`` = AttLayer(z) [B, 6]) and
``g<c>`` (the gradients of ``sum(y * up)`` with respect to ``x`` and the three parameters).  A seed is refused when a
pre-activation of the attention layer lies within 1e-4 of zero, so that fp32 rounding on another device cannot flip a unit.
Data only.

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

CASES = ((37, 5, 8, 25), (19, 7, 16, 32))
MIN_PRE_RELU = 1e-4


def _offline():
    def refuse(*a, **k):
        raise OSError("offline")
    req = types.ModuleType("requests")
    req.get = refuse
    sys.modules["requests"] = req
    sys.modules["recbox.third_party.deepctr"] = types.ModuleType("recbox.third_party.deepctr")


class _Host(object):
    """What ``AFM.afm_layer`` reads of its model."""


def record(c, dims, L, AFM, out):
    B, F, D, A = dims
    for seed in range(100 + c, 300, 2):
        g = torch.Generator().manual_seed(seed)
        host = _Host()
        host.num_feature_field = F
        host.attlayer = L.AttLayer(D, A)
        host.p = torch.nn.Parameter(torch.randn(D, generator=g))
        host.dropout_layer = torch.nn.Dropout(p=0.0)
        host.build_cross = lambda feat_emb, host=host: AFM.build_cross(host, feat_emb)
        with torch.no_grad():
            host.attlayer.w.weight.copy_(torch.randn(A, D, generator=g) * 0.5)
            host.attlayer.h.copy_(torch.randn(A, generator=g))
        x = torch.randn(B, F, D, generator=g).requires_grad_()
        up = torch.randn(B, 1, generator=g)
        z = torch.randn(B, 6, D, generator=g)
        left, right = host.build_cross(x)
        pair = (left * right).detach()
        closest = float(host.attlayer.w(pair).detach().abs().min())
        if closest > MIN_PRE_RELU:
            break
    else:
        raise RuntimeError("no seed keeps every pre-activation away from zero for %s" % (dims,))
    y = AFM.afm_layer(host, x)
    assert tuple(y.shape) == (B, 1)
    (y * up).sum().backward()
    with torch.no_grad():
        att, att_z = host.attlayer(pair), host.attlayer(z)
    print("case %d %s: seed %d, smallest |pre-activation| %.2e" % (c, dims, seed, closest))
    params = {"attlayer.w.weight": host.attlayer.w.weight, "attlayer.h": host.attlayer.h, "p": host.p}
    assert sorted(host.attlayer.state_dict().keys()) == ["h", "w.weight"]
    out.update({"in%d.x" % c: x.detach().numpy(), "in%d.up" % c: up.numpy(), "in%d.z" % c: z.numpy(),
                "out%d.y" % c: y.detach().numpy(), "out%d.att" % c: att.numpy(), "out%d.att_z" % c: att_z.numpy(),
                "g%d.x" % c: x.grad.numpy()})
    for k, v in params.items():
        out["p%d.%s" % (c, k)] = v.detach().numpy()
        out["g%d.%s" % (c, k)] = v.grad.numpy()


def main():
    _offline()
    import gen_golden_recbole
    L = gen_golden_recbole.recbole_layers()
    import importlib
    AFM = importlib.import_module("recbox.third_party.recbole.model.context_aware_recommender.afm").AFM
    out = {}
    for c, dims in enumerate(CASES):
        record(c, dims, L, AFM, out)
    path = os.path.join(ROOT, "tests", "golden", "afm.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d arrays, %d bytes)" % (path, len(out), os.path.getsize(path)))
    assert os.path.getsize(path) < 100 * 1024


if __name__ == "__main__":
    main()
