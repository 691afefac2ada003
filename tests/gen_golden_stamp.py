"""Generate tests/golden/rechub_stamp.npz from the LIVE reference (dev container only; run from the repository root):

    python tests/gen_golden_stamp.py

STAMP (third_party/rechub/models/matching/stamp.py) at B = 16, L = 6, embed 8, 23 items; sessions left-aligned (id 0 =
padding) with lengths 1..6, among them several of length 1 and several full ones.  Seeded non-zero parameters, ``b_a`` and the
table's padding row included (the reference's own initialisation overwrites that row too).  Groups: ``in`` (``session``),
``p_stamp`` (state_dict), ``out_stamp`` (the score matrix ``z``) and ``g_stamp`` (parameter gradients of z.sum()).  Data only."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, L, D, N_ITEMS = 16, 6, 8, 23


def main():
    from oracle import ref_shim
    ref_shim.import_reference()
    import torch_rechub.basic.features as feats
    from recbox.third_party.rechub.models.matching.stamp import STAMP

    g = torch.Generator().manual_seed(20263)
    lengths = torch.tensor([6, 1, 2, 3, 4, 5, 6, 1, 3, 6, 2, 5, 4, 6, 1, 3])
    session = torch.randint(1, N_ITEMS, (B, L), generator=g)
    session = session * (torch.arange(L).unsqueeze(0) < lengths.unsqueeze(1))
    out = {"in.session": session.numpy()}
    model = STAMP(feats.SequenceFeature("session", vocab_size=N_ITEMS, embed_dim=D, pooling="concat"), 0.3, 0.5)
    with torch.no_grad():
        for name, p in model.named_parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (0.5 if "emb" in name else 0.3))
    model.train()
    for k, v in model.state_dict().items():
        out["p_stamp." + k] = v.detach().clone().numpy()
    z = model({"session": session})
    z.sum().backward()
    assert tuple(z.shape) == (B, N_ITEMS)
    out["out_stamp.z"] = z.detach().numpy()
    for name, p in model.named_parameters():
        out["g_stamp." + name] = (p.grad if p.grad is not None else torch.zeros_like(p)).numpy()
    path = os.path.join(ROOT, "tests", "golden", "rechub_stamp.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d arrays, %d bytes)" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
