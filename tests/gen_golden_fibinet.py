"""Generate tests/golden/rechub_fibinet.npz from the LIVE reference (dev container only; run from the repository root):

    python tests/gen_golden_fibinet.py

FiBiNet (third_party/rechub/models/ranking/fibinet.py) with F = 5 sparse features of dim D = 8 at B = 6, once per bilinear type
(field_all, field_each, field_interaction): reduction_ratio 3 (one hidden unit in the gate), an MLP of dims [4] with ReLU,
dropout 0, seeded non-zero parameters (BatchNorm affine terms included), ``model.train()``.  Groups: ``in`` (ids) and per type
``p_*`` (state_dict), ``keys`` (the ordered state_dict keys), ``out_*`` (y) and ``g_*`` (parameter gradients of y.sum()).  The
two layers alone, on ``layer.x`` [B, F, D]: ``senet`` (its two weights and ``out``) and ``bi_<type>`` (its state_dict,
``keys_bi`` and ``out``).  A seed is refused when any value entering a ReLU lies within 1e-4 of zero, so that fp32 rounding on
another device cannot flip a unit.  Data only."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, F, D = 6, 5, 8
VOCABS = (11, 7, 13, 5, 9)
KINDS = ("field_all", "field_each", "field_interaction")
MIN_PRE_RELU = 1e-4


def build(kind, mod, cls):
    """FiBiNet of ``kind`` over fresh feature objects of ``mod`` (the reference's feature module or this package's)."""
    feats = [mod.SparseFeature("s%d" % i, vocab_size=v, embed_dim=D) for i, v in enumerate(VOCABS)]
    return cls(feats, {"dims": [4], "activation": "relu", "dropout": 0.0}, reduction_ratio=3, bilinear_type=kind)


def inputs(g):
    return {"s%d" % i: torch.randint(0, v, (B,), generator=g) for i, v in enumerate(VOCABS)}


def seed_params(model, g):
    with torch.no_grad():
        for name, p in model.named_parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (0.5 if "embed" in name else 0.4))
            if p.dim() == 1 and name.endswith(".weight"):                       # BatchNorm scales: around 1
                p.add_(1.0)
            if "senet" in name:                                                 # a gate that opens for some fields
                p.abs_()


def run(model, x):
    """(y, {parameter: gradient of y.sum()}, smallest |value| entering a ReLU)"""
    closest = [float("inf")]

    def watch(_, args):
        closest[0] = min(closest[0], args[0].detach().abs().min().item())

    hooks = [m.register_forward_pre_hook(watch) for m in model.modules() if isinstance(m, torch.nn.ReLU)]
    model.train()
    model.zero_grad()
    y = model(x)
    y.sum().backward()
    for h in hooks:
        h.remove()
    grads = {n: (p.grad if p.grad is not None else torch.zeros_like(p)).clone() for n, p in model.named_parameters()}
    return y.detach(), grads, closest[0]


def main():
    from oracle import ref_shim
    # the reference's vendored deepctr asks a package index for its latest version when imported; generation runs offline
    offline = types.ModuleType("requests")
    offline.get = lambda *a, **k: (_ for _ in ()).throw(OSError("offline"))
    sys.modules.setdefault("requests", offline)
    ref_shim.import_reference()
    import recbox.third_party.rechub.basic.features as feats
    from recbox.third_party.rechub.basic.layers import BiLinearInteractionLayer, SENETLayer
    from recbox.third_party.rechub.models.ranking.fibinet import FiBiNet

    x = inputs(torch.Generator().manual_seed(20267))
    out = {"in." + n: t.numpy() for n, t in x.items()}
    for kind in KINDS:
        for seed in range(500, 700):
            model = build(kind, feats, FiBiNet)
            assert model.senet_layer.mlp[0].weight.shape == (1, F) and model.dims == F * (F - 1) * D
            seed_params(model, torch.Generator().manual_seed(seed))
            params = {k: v.detach().clone() for k, v in model.state_dict().items()}
            y, grads, closest = run(model, x)
            if closest > MIN_PRE_RELU:
                break
        else:
            raise RuntimeError("no seed keeps every pre-ReLU value away from zero for " + kind)
        print("%s: seed %d, smallest |pre-ReLU| %.2e, y %s" % (kind, seed, closest, tuple(y.shape)))
        out["keys." + kind] = np.array(list(params.keys()))
        for k, v in params.items():
            out["p_%s.%s" % (kind, k)] = v.numpy()
        out["out_%s.y" % kind] = y.numpy()
        for k, v in grads.items():
            out["g_%s.%s" % (kind, k)] = v.numpy()

    g = torch.Generator().manual_seed(77)
    lx = torch.randn(B, F, D, generator=g) * 0.7 + 0.3
    out["layer.x"] = lx.numpy()
    senet = SENETLayer(F, 3)
    with torch.no_grad():
        for p in senet.parameters():
            p.copy_(torch.rand(p.shape, generator=g) - 0.3)
    with torch.no_grad():
        sv = senet(lx)
    assert (sv == 0).any() and (sv != 0).any()                                  # a closed and an open field
    for k, v in senet.state_dict().items():
        out["senet." + k] = v.numpy()
    out["senet.out"] = sv.numpy()
    for kind in KINDS:
        layer = BiLinearInteractionLayer(D, F, kind)
        with torch.no_grad():
            for p in layer.parameters():
                p.copy_(torch.randn(p.shape, generator=g) * 0.4)
            out["bi_%s.out" % kind] = layer(lx).numpy()
        out["keys_bi." + kind] = np.array(list(layer.state_dict().keys()))
        for k, v in layer.state_dict().items():
            out["bi_%s.%s" % (kind, k)] = v.numpy()
    path = os.path.join(ROOT, "tests", "golden", "rechub_fibinet.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d arrays, %d bytes)" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
