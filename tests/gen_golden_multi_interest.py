"""Generate tests/golden/rechub_multi_interest.npz from the LIVE reference (dev container only; run from the repository
root):

    python tests/gen_golden_multi_interest.py

MIND and ComirecDR (third_party/rechub/models/matching/mind.py, comirec.py) at B = 16, L = 6, D = 8, K = 3: one user
feature, one item table shared by the history (pooling "concat"), the target and 3 negatives; histories of lengths 0..6
(id 0 = padding, at least one history empty); seeded non-zero parameters.  ``torch.manual_seed(SEED)`` is called just
before each forward, and MIND's starting logits are stored as what ``torch.randn(B, K, L)`` returns after the same
re-seed.  Groups: ``in`` (ids), ``extra`` (MIND's start), and per model ``p_*`` (state_dict), ``out_*`` (y and the
mode="user" output) and ``g_*`` (parameter gradients of y.sum()).  Data only."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, L, D, K, N_NEG = 16, 6, 8, 3, 3
N_USERS, N_ITEMS = 11, 23
SEED = 77


def features(mod):
    user = [mod.SparseFeature("user_id", vocab_size=N_USERS, embed_dim=D)]
    hist = [mod.SequenceFeature("hist_item_id", vocab_size=N_ITEMS, embed_dim=D, pooling="concat", shared_with="item_id")]
    item = [mod.SparseFeature("item_id", vocab_size=N_ITEMS, embed_dim=D)]
    neg = [mod.SequenceFeature("neg_items", vocab_size=N_ITEMS, embed_dim=D, pooling="concat", shared_with="item_id")]
    return user, hist, item, neg


def main():
    from oracle import ref_shim
    ref_shim.import_reference()
    import torch_rechub.basic.features as feats
    from recbox.third_party.rechub.models.matching.mind import MIND
    from recbox.third_party.rechub.models.matching.comirec import ComirecDR

    g = torch.Generator().manual_seed(20261)
    lengths = torch.tensor([0, 6, 1, 2, 3, 4, 5, 6, 0, 3, 6, 1, 5, 2, 4, 6])
    hist = torch.randint(1, N_ITEMS, (B, L), generator=g)
    hist = hist * (torch.arange(L).unsqueeze(0) < lengths.unsqueeze(1))
    x = {"user_id": torch.randint(0, N_USERS, (B,), generator=g), "hist_item_id": hist,
         "item_id": torch.randint(1, N_ITEMS, (B,), generator=g), "neg_items": torch.randint(1, N_ITEMS, (B, N_NEG), generator=g)}
    out = {"in." + n: t.numpy() for n, t in x.items()}
    torch.manual_seed(SEED)
    out["extra.mind_start"] = torch.randn(B, K, L).numpy()
    for tag, cls in (("mind", MIND), ("comirec", ComirecDR)):
        model = cls(*features(feats), max_length=L, interest_num=K)
        with torch.no_grad():
            for name, p in model.named_parameters():
                p.copy_(torch.randn(p.shape, generator=g) * (0.5 if "embed_dict" in name else 0.3))
        model.train()
        for k, v in model.state_dict().items():
            out["p_%s.%s" % (tag, k)] = v.detach().clone().numpy()
        model.mode = "user"
        torch.manual_seed(SEED)
        out["out_%s.user" % tag] = model(x).detach().numpy()
        model.mode = None
        torch.manual_seed(SEED)
        y = model(x)
        y.sum().backward()
        assert tuple(y.shape) == (B, D)
        out["out_%s.y" % tag] = y.detach().numpy()
        for name, p in model.named_parameters():
            out["g_%s.%s" % (tag, name)] = (p.grad if p.grad is not None else torch.zeros_like(p)).numpy()
    path = os.path.join(ROOT, "tests", "golden", "rechub_multi_interest.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d arrays, %d bytes)" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
