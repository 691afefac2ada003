"""Generate tests/golden/rechub_deepffm.npz from the LIVE reference (dev container only; run from the repository root):

    python tests/gen_golden_deepffm.py

DeepFFM and FatDeepFFM (third_party/rechub/models/ranking/deepffm.py) with F = 4 cross features of D = 8, vocabularies
3 / 5 / 7 / 11 (tables of vocab * F rows), B = 16, MLP dims [16, 8], dropout 0, reduction_ratio 2, seeded non-zero
parameters, in training mode (BatchNorm on batch statistics).  Groups: ``in`` (ids), and per model ``p_*`` (state_dict),
``out_*`` (y) and ``g_*`` (parameter gradients of y.sum()).  Data only."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F, D, B = 4, 8, 16
VOCABS = [3, 5, 7, 11]
NAMES = ["C%d" % i for i in range(F)]


def main():
    from oracle import ref_shim
    ref_shim.import_reference()
    from torch_rechub.basic.features import SparseFeature
    from recbox.third_party.rechub.models.ranking.deepffm import DeepFFM, FatDeepFFM

    g = torch.Generator().manual_seed(20260)
    x = {n: torch.randint(0, v, (B,), generator=g) for n, v in zip(NAMES, VOCABS)}
    out = {"in." + n: t.numpy() for n, t in x.items()}
    for tag, fat in (("deep", False), ("fat", True)):
        linear = [SparseFeature(n, vocab_size=v, embed_dim=1) for n, v in zip(NAMES, VOCABS)]
        crossf = [SparseFeature(n, vocab_size=v * F, embed_dim=D) for n, v in zip(NAMES, VOCABS)]
        mlp = {"dims": [16, 8], "dropout": 0.0, "activation": "relu"}
        model = FatDeepFFM(linear, crossf, D, 2, mlp) if fat else DeepFFM(linear, crossf, D, mlp)
        with torch.no_grad():
            for name, p in model.named_parameters():
                scale = 0.5 if "embed_dict" in name else 0.3
                p.copy_(torch.randn(p.shape, generator=g) * scale)
                if name.endswith("u"):
                    p.abs_()
        model.train()
        for k, v in model.state_dict().items():
            out["p_%s.%s" % (tag, k)] = v.detach().clone().numpy()
        y = model(x)
        y.sum().backward()
        out["out_%s.y" % tag] = y.detach().numpy()
        for name, p in model.named_parameters():
            out["g_%s.%s" % (tag, name)] = (p.grad if p.grad is not None else torch.zeros_like(p)).numpy()
    path = os.path.join(ROOT, "tests", "golden", "rechub_deepffm.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d arrays, %d bytes)" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
