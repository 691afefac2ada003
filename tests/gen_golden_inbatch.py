"""Generate tests/golden/rechub_inbatch.npz from the LIVE reference (dev container only; run from the repository root):

    python tests/gen_golden_inbatch.py

``sbc``: third_party/rechub/models/matching/youtube_sbc.py YoutubeSBC with batch_size 6, n_neg 3, temperature 0.5, two sparse
user features, two sparse item features, one DenseFeature sample weight in [0.05, 1], towers [8] with ReLU, dropout 0,
``model.train()``: a full batch of 6 rows and, on a FRESH model with the same parameters, a short batch of 5 rows (the
reference writes into its stored index on a short batch, so the order of calls matters there).  ``fb``:
models/matching/dssm_facebook.py FaceBookDSSM at B = 6 over the same user and item groups, the negative item features sharing
the positive ones' tables.  Groups: ``in_<model>_<batch>`` (inputs), ``up_<model>_<batch>`` (the seeded weights of the loss
``sum(output * up)``), ``p_<model>`` (state_dict), ``keys`` (ordered state_dict keys), ``out_<model>_<batch>`` (outputs),
``g_<model>_<batch>`` (parameter gradients of the loss), ``mode_<model>`` (the ``user`` / ``item`` mode outputs on the full batch)
and ``loss`` (HingeLoss() and BPRLoss() of basic/loss_func.py on recorded score vectors).  A seed is refused when any value
entering a ReLU lies within 1e-4 of zero, so that fp32 rounding on another device cannot flip a unit.  Data only."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, SHORT, N_NEG, TEMPERATURE, D = 6, 5, 3, 0.5, 4
USER_VOCABS, ITEM_VOCABS = (11, 7), (13, 5)
MIN_PRE_RELU = 1e-4


def build(which, feats_mod, models):
    """Model ``which`` over fresh feature objects of ``feats_mod``; ``models`` has YoutubeSBC and FaceBookDSSM."""
    user = [feats_mod.SparseFeature("u%d" % i, vocab_size=v, embed_dim=D) for i, v in enumerate(USER_VOCABS)]
    item = [feats_mod.SparseFeature("i%d" % i, vocab_size=v, embed_dim=D) for i, v in enumerate(ITEM_VOCABS)]
    tower = lambda: {"dims": [8], "activation": "relu", "dropout": 0.0}             # noqa: E731
    if which == "sbc":
        return models.YoutubeSBC(user, item, [feats_mod.DenseFeature("sw")], tower(), tower(), batch_size=B, n_neg=N_NEG,
                                 temperature=TEMPERATURE)
    if which == "fb":
        neg = [feats_mod.SparseFeature("neg_i%d" % i, vocab_size=v, embed_dim=D, shared_with="i%d" % i)
               for i, v in enumerate(ITEM_VOCABS)]
        return models.FaceBookDSSM(user, item, neg, tower(), tower())
    raise ValueError(which)


def inputs(which, rows, g):
    x = {"u%d" % i: torch.randint(0, v, (rows,), generator=g) for i, v in enumerate(USER_VOCABS)}
    x.update({"i%d" % i: torch.randint(0, v, (rows,), generator=g) for i, v in enumerate(ITEM_VOCABS)})
    if which == "sbc":
        x["sw"] = 0.05 + 0.95 * torch.rand(rows, generator=g)
    else:
        x.update({"neg_i%d" % i: torch.randint(0, v, (rows,), generator=g) for i, v in enumerate(ITEM_VOCABS)})
    return x


def outputs(which, result):
    return {"scores": result} if which == "sbc" else {"pos": result[0], "neg": result[1]}


def loss(which, outs, up):
    return sum((outs[k] * up[k]).sum() for k in sorted(outs))


def seed_params(model, g):
    with torch.no_grad():
        for name, p in model.named_parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (0.5 if "embed" in name else 0.4))
            if p.dim() == 1 and name.endswith(".weight"):                       # BatchNorm scales: around 1
                p.add_(1.0)


def run(which, model, x, up):
    """({output: tensor}, {parameter: gradient of the loss}, smallest |value| entering a ReLU)"""
    closest = [float("inf")]

    def watch(_, args):
        closest[0] = min(closest[0], args[0].detach().abs().min().item())

    hooks = [m.register_forward_pre_hook(watch) for m in model.modules() if isinstance(m, torch.nn.ReLU)]
    model.train()
    model.zero_grad()
    outs = outputs(which, model(x))
    loss(which, outs, up).backward()
    for h in hooks:
        h.remove()
    grads = {n: (p.grad if p.grad is not None else torch.zeros_like(p)).clone() for n, p in model.named_parameters()}
    return {k: t.detach().clone() for k, t in outs.items()}, grads, closest[0]


def main():
    from oracle import ref_shim
    # the reference's vendored deepctr asks a package index for its latest version when imported; generation runs offline
    offline = types.ModuleType("requests")
    offline.get = lambda *a, **k: (_ for _ in ()).throw(OSError("offline"))
    sys.modules.setdefault("requests", offline)
    ref_shim.import_reference()
    import recbox.third_party.rechub.basic.features as feats
    from recbox.third_party.rechub.basic.loss_func import BPRLoss, HingeLoss
    from recbox.third_party.rechub.models.matching.dssm_facebook import FaceBookDSSM
    from recbox.third_party.rechub.models.matching.youtube_sbc import YoutubeSBC
    models = types.SimpleNamespace(YoutubeSBC=YoutubeSBC, FaceBookDSSM=FaceBookDSSM)

    out = {}
    g = torch.Generator().manual_seed(20271)
    batches = {"sbc": {"full": inputs("sbc", B, g), "short": inputs("sbc", SHORT, g)}, "fb": {"full": inputs("fb", B, g)}}
    ups = {"sbc": {"full": {"scores": torch.randn(B, N_NEG + 1, generator=g)}, "short": {"scores": torch.randn(SHORT, N_NEG + 1, generator=g)}},
           "fb": {"full": {"pos": torch.randn(B, generator=g), "neg": torch.randn(B, generator=g)}}}
    for which in ("sbc", "fb"):
        for seed in range(900, 1100):
            results, closest = {}, float("inf")
            for tag, x in batches[which].items():
                model = build(which, feats, models)                           # fresh: the reference's short batch writes its index
                seed_params(model, torch.Generator().manual_seed(seed))
                params = {k: v.detach().clone() for k, v in model.state_dict().items()}
                outs, grads, c = run(which, model, x, ups[which][tag])
                results[tag] = (outs, grads)
                closest = min(closest, c)
            if closest > MIN_PRE_RELU:
                break
        else:
            raise RuntimeError("no seed keeps every pre-ReLU value away from zero for " + which)
        print("%s: seed %d, smallest |pre-ReLU| %.2e" % (which, seed, closest))
        out["keys." + which] = np.array(list(params.keys()))
        out["seed." + which] = np.array([seed, closest])
        for k, v in params.items():
            out["p_%s.%s" % (which, k)] = v.numpy()
        for tag, (outs, grads) in results.items():
            for k, v in batches[which][tag].items():
                out["in_%s_%s.%s" % (which, tag, k)] = v.numpy()
            for k, v in ups[which][tag].items():
                out["up_%s_%s.%s" % (which, tag, k)] = v.numpy()
            for k, v in outs.items():
                out["out_%s_%s.%s" % (which, tag, k)] = v.numpy()
            for k, v in grads.items():
                out["g_%s_%s.%s" % (which, tag, k)] = v.numpy()
        for mode in ("user", "item"):
            model = build(which, feats, models)
            model.load_state_dict(params)
            model.train()
            model.mode = mode
            out["mode_%s.%s" % (which, mode)] = model(batches[which]["full"]).detach().numpy()

    pos, neg = torch.randn(B, generator=g), torch.randn(B, N_NEG, generator=g)
    out.update({"loss.pos": pos.numpy(), "loss.neg": neg.numpy(), "loss.hinge": HingeLoss()(pos, neg).numpy(),
                "loss.bpr_pairs": BPRLoss()(pos, neg[:, 0]).numpy(), "loss.bpr_rows": BPRLoss()(pos.view(-1, 1), neg).numpy()})
    path = os.path.join(ROOT, "tests", "golden", "rechub_inbatch.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d arrays, %d bytes)" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
