"""Generate tests/golden/rechub_dcn.npz from the LIVE reference (dev container only; run from the repository root):

    python tests/gen_golden_crossmix.py

The Deep & Cross family of third_party/rechub/models/ranking over F = 5 sparse features of dim 8 at B = 6: ``dcn`` (DCN),
``v2par`` / ``v2stk`` (DCNv2 parallel / stacked with the low-rank mixture, low_rank 4, 3 experts), ``v2only`` (DCNv2
crossnet_only with CrossNetV2), ``edcn_h`` (EDCN, hadamard_product bridge, with regulation), ``edcn_a`` (EDCN,
attention_pooling bridge, without) and ``wd`` (WideDeep: features 0..1 wide, 2..4 deep).  2 cross layers, MLP dims [4] with
ReLU, dropout 0, seeded non-zero parameters (BatchNorm affine terms and the cross biases included), ``model.train()``.  Groups:
``in`` (ids) and per model ``p_*`` (state_dict), ``keys`` (the ordered state_dict keys), ``out_*`` (y) and ``g_*`` (parameter
gradients of y.sum()).  A seed is refused when any value entering a ReLU lies within 1e-4 of zero, so that fp32 rounding on
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
MODELS = ("dcn", "v2par", "v2stk", "v2only", "edcn_h", "edcn_a", "wd")
MIN_PRE_RELU = 1e-4


def build(which, feats_mod, models):
    """Model ``which`` over fresh feature objects of ``feats_mod``; ``models`` has DCN, DCNv2, EDCN and WideDeep."""
    feats = [feats_mod.SparseFeature("s%d" % i, vocab_size=v, embed_dim=D) for i, v in enumerate(VOCABS)]
    mlp = {"dims": [4], "activation": "relu", "dropout": 0.0}
    if which == "dcn":
        return models.DCN(feats, 2, mlp)
    if which in ("v2par", "v2stk"):
        return models.DCNv2(feats, 2, mlp, model_structure="parallel" if which == "v2par" else "stacked",
                            use_low_rank_mixture=True, low_rank=4, num_experts=3)
    if which == "v2only":
        return models.DCNv2(feats, 2, mlp, model_structure="crossnet_only", use_low_rank_mixture=False)
    if which == "edcn_h":
        return models.EDCN(feats, 2, mlp, bridge_type="hadamard_product", use_regulation_module=True)
    if which == "edcn_a":
        return models.EDCN(feats, 2, mlp, bridge_type="attention_pooling", use_regulation_module=False)
    if which == "wd":
        return models.WideDeep(feats[:2], feats[2:], mlp)
    raise ValueError(which)


def inputs(g):
    return {"s%d" % i: torch.randint(0, v, (B,), generator=g) for i, v in enumerate(VOCABS)}


def seed_params(model, g):
    with torch.no_grad():
        for name, p in model.named_parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (0.5 if "embed" in name else 0.4))
            if p.dim() == 1 and name.endswith(".weight"):                       # BatchNorm scales: around 1
                p.add_(1.0)


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
    from recbox.third_party.rechub.models.ranking.dcn import DCN
    from recbox.third_party.rechub.models.ranking.dcn_v2 import DCNv2
    from recbox.third_party.rechub.models.ranking.edcn import EDCN
    from recbox.third_party.rechub.models.ranking.widedeep import WideDeep
    models = types.SimpleNamespace(DCN=DCN, DCNv2=DCNv2, EDCN=EDCN, WideDeep=WideDeep)

    x = inputs(torch.Generator().manual_seed(20268))
    out = {"in." + n: t.numpy() for n, t in x.items()}
    for which in MODELS:
        for seed in range(800, 1000):
            model = build(which, feats, models)
            seed_params(model, torch.Generator().manual_seed(seed))
            params = {k: v.detach().clone() for k, v in model.state_dict().items()}
            y, grads, closest = run(model, x)
            if closest > MIN_PRE_RELU:
                break
        else:
            raise RuntimeError("no seed keeps every pre-ReLU value away from zero for " + which)
        print("%s: seed %d, smallest |pre-ReLU| %.2e, y %s" % (which, seed, closest, tuple(y.shape)))
        out["keys." + which] = np.array(list(params.keys()))
        for k, v in params.items():
            out["p_%s.%s" % (which, k)] = v.numpy()
        out["out_%s.y" % which] = y.numpy()
        out["seed." + which] = np.array([seed, closest])
        for k, v in grads.items():
            out["g_%s.%s" % (which, k)] = v.numpy()
    path = os.path.join(ROOT, "tests", "golden", "rechub_dcn.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d arrays, %d bytes)" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
