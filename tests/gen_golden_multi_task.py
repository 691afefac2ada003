"""Generate tests/golden/rechub_multi_task.npz from the LIVE reference (dev container only; run from the repository root):

    python tests/gen_golden_multi_task.py

SharedBottom, ESMM, MMOE, PLE and AITM (third_party/rechub/models/multi_task/) at B = 16: three sparse features of dim 4, one
mean-pooled sequence feature of dim 4 and L = 5 (id 0 = padding, lengths 0 .. 5) and one dense feature; all dropouts 0, seeded
non-zero parameters (BatchNorm affine terms included), ``model.train()``.  MMOE: 3 experts of dims [8, 6], tasks
(classification, regression), towers [4].  PLE: 2 levels, 2 specific + 1 shared experts of dims [6], towers [4].  AITM: 3
tasks, bottoms [8], towers [4].  SharedBottom: bottom [8], towers [4]; ESMM: user = (one sparse, the sequence), item = (two
sparse), towers [4].  Groups: ``in`` (ids and values) and per model ``p_*`` (state_dict), ``out_*`` (y), ``g_*`` (parameter
gradients of y.sum()) and ``keys`` (the ordered state_dict keys).  A seed is refused when any value entering a ReLU lies
within 1e-5 of zero, so that fp32 rounding on another device cannot flip a unit.  Data only."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, L, D = 16, 5, 4
VOCABS = (11, 7, 13)
N_TAGS = 9
MIN_PRE_RELU = 1e-5
TAGS = ("shared_bottom", "esmm", "mmoe", "ple", "aitm")


def features(mod):
    sparse = [mod.SparseFeature("s%d" % i, vocab_size=v, embed_dim=D) for i, v in enumerate(VOCABS)]
    seq = mod.SequenceFeature("tags", vocab_size=N_TAGS, embed_dim=D, pooling="mean", padding_idx=0)
    return sparse, seq, mod.DenseFeature("price")


def build(tag, mod, models):
    """The model ``tag`` over fresh feature objects of ``mod`` (the reference's feature module or this package's)."""
    sparse, seq, dense = features(mod)
    feats = sparse + [seq, dense]
    tower = {"dims": [4], "activation": "relu", "dropout": 0.0}
    if tag == "shared_bottom":
        return models["SharedBottom"](feats, ["classification", "regression"], {"dims": [8], "activation": "relu", "dropout": 0.0},
                                      [dict(tower), dict(tower)])
    if tag == "esmm":
        return models["ESMM"]([sparse[0], seq], sparse[1:], dict(tower), dict(tower))
    if tag == "mmoe":
        return models["MMOE"](feats, ["classification", "regression"], 3, {"dims": [8, 6], "activation": "relu", "dropout": 0.0},
                              [dict(tower), dict(tower)])
    if tag == "ple":
        return models["PLE"](feats, ["classification", "regression"], 2, 2, 1, {"dims": [6], "activation": "relu", "dropout": 0.0},
                             [dict(tower), dict(tower)])
    if tag == "aitm":
        return models["AITM"](feats, 3, {"dims": [8], "activation": "relu", "dropout": 0.0}, [dict(tower) for _ in range(3)])
    raise KeyError(tag)


def inputs(g):
    lengths = torch.tensor([5, 0, 1, 2, 3, 4, 5, 1, 0, 3, 2, 5, 4, 1, 3, 2])
    tags = torch.randint(1, N_TAGS, (B, L), generator=g) * (torch.arange(L).unsqueeze(0) < lengths.unsqueeze(1))
    x = {"s%d" % i: torch.randint(0, v, (B,), generator=g) for i, v in enumerate(VOCABS)}
    x["tags"] = tags
    x["price"] = torch.rand(B, generator=g)
    return x


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
    import torch_rechub.basic.features as feats
    from recbox.third_party.rechub.models.multi_task.aitm import AITM
    from recbox.third_party.rechub.models.multi_task.esmm import ESMM
    from recbox.third_party.rechub.models.multi_task.mmoe import MMOE
    from recbox.third_party.rechub.models.multi_task.ple import PLE
    from recbox.third_party.rechub.models.multi_task.shared_bottom import SharedBottom
    models = {"SharedBottom": SharedBottom, "ESMM": ESMM, "MMOE": MMOE, "PLE": PLE, "AITM": AITM}

    x = inputs(torch.Generator().manual_seed(20263))
    assert (x["tags"] == 0).all(dim=1).sum() >= 2 and (x["tags"] != 0).all(dim=1).sum() >= 2
    out = {"in." + n: t.numpy() for n, t in x.items()}
    for tag in TAGS:
        for seed in range(300, 400):
            model = build(tag, feats, models)
            seed_params(model, torch.Generator().manual_seed(seed))
            params = {k: v.detach().clone() for k, v in model.state_dict().items()}
            y, grads, closest = run(model, x)
            if closest > MIN_PRE_RELU:
                break
        else:
            raise RuntimeError("no seed keeps every pre-ReLU value away from zero for " + tag)
        print("%s: seed %d, smallest |pre-ReLU| %.2e, y %s" % (tag, seed, closest, tuple(y.shape)))
        out["keys." + tag] = np.array(list(params.keys()))
        for k, v in params.items():
            out["p_%s.%s" % (tag, k)] = v.numpy()
        out["out_%s.y" % tag] = y.numpy()
        for k, v in grads.items():
            out["g_%s.%s" % (tag, k)] = v.numpy()
    assert np.array_equal(out["out_esmm.y"][:, 2], out["out_esmm.y"][:, 0] ** 2)
    path = os.path.join(ROOT, "tests", "golden", "rechub_multi_task.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d arrays, %d bytes)" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
