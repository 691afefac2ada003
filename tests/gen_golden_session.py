"""Generate tests/golden/rechub_session.npz from the LIVE reference (dev container only; run from the repository root):

    python tests/gen_golden_session.py

GRU4Rec and NARM (third_party/rechub/models/matching/gru4rec.py, narm.py) at B = 16, L = 6, embed 8.  GRU4Rec: one user
feature, one item table shared by the history (pooling "concat"), the target and 3 negatives, a 2-layer bias-free GRU, a
user tower of one layer of 8 units without dropout.  NARM: hidden 12, both dropouts 0; sessions left-aligned (id 0 =
padding) with lengths 1..6, several of length 6 (the reference's attention broadcasts only with a full-length session in the
batch).  Seeded non-zero parameters.  Groups: ``in`` (ids; NARM's sessions under ``session``), and per model ``p_*``
(state_dict), ``out_*`` (y and the mode="user" output for GRU4Rec, the score matrix ``s`` for NARM) and ``g_*`` (parameter
gradients of y.sum() / s.sum()).  Data only."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, L, D, HID, N_NEG = 16, 6, 8, 12, 3
N_USERS, N_ITEMS = 11, 23


def gru4rec_features(mod):
    user = [mod.SparseFeature("user_id", vocab_size=N_USERS, embed_dim=D)]
    hist = [mod.SequenceFeature("hist_item_id", vocab_size=N_ITEMS, embed_dim=D, pooling="concat", shared_with="item_id")]
    item = [mod.SparseFeature("item_id", vocab_size=N_ITEMS, embed_dim=D)]
    neg = [mod.SequenceFeature("neg_items", vocab_size=N_ITEMS, embed_dim=D, pooling="concat", shared_with="item_id")]
    return user, hist, item, neg


def narm_feature(mod):
    return mod.SequenceFeature("session", vocab_size=N_ITEMS, embed_dim=D, pooling="concat")


def main():
    from oracle import ref_shim
    ref_shim.import_reference()
    import torch_rechub.basic.features as feats
    from recbox.third_party.rechub.models.matching.gru4rec import GRU4Rec
    from recbox.third_party.rechub.models.matching.narm import NARM

    g = torch.Generator().manual_seed(20262)
    lengths = torch.tensor([6, 1, 2, 3, 4, 5, 6, 1, 3, 6, 2, 5, 4, 6, 1, 3])
    session = torch.randint(1, N_ITEMS, (B, L), generator=g)
    session = session * (torch.arange(L).unsqueeze(0) < lengths.unsqueeze(1))
    x = {"user_id": torch.randint(0, N_USERS, (B,), generator=g), "hist_item_id": torch.randint(1, N_ITEMS, (B, L), generator=g),
         "item_id": torch.randint(1, N_ITEMS, (B,), generator=g), "neg_items": torch.randint(1, N_ITEMS, (B, N_NEG), generator=g),
         "session": session}
    out = {"in." + n: t.numpy() for n, t in x.items()}

    def fill(model):
        with torch.no_grad():
            for name, p in model.named_parameters():
                p.copy_(torch.randn(p.shape, generator=g) * (0.5 if "emb" in name else 0.3))
        model.train()

    model = GRU4Rec(*gru4rec_features(feats), user_params={"dims": [D], "activation": "relu", "dropout": 0.0})
    fill(model)
    for k, v in model.state_dict().items():
        out["p_gru4rec." + k] = v.detach().clone().numpy()
    model.mode = "user"
    out["out_gru4rec.user"] = model(x).detach().numpy()
    model.load_state_dict({k[len("p_gru4rec."):]: torch.from_numpy(v) for k, v in out.items() if k.startswith("p_gru4rec.")})
    model.mode = None
    y = model(x)
    y.sum().backward()
    assert tuple(y.shape) == (B, D)
    out["out_gru4rec.y"] = y.detach().numpy()
    for name, p in model.named_parameters():
        out["g_gru4rec." + name] = (p.grad if p.grad is not None else torch.zeros_like(p)).numpy()

    model = NARM(narm_feature(feats), HID, 0.0, 0.0)
    fill(model)
    for k, v in model.state_dict().items():
        out["p_narm." + k] = v.detach().clone().numpy()
    s = model({"session": session})
    s.sum().backward()
    assert tuple(s.shape) == (B, N_ITEMS)
    out["out_narm.s"] = s.detach().numpy()
    for name, p in model.named_parameters():
        out["g_narm." + name] = (p.grad if p.grad is not None else torch.zeros_like(p)).numpy()
    path = os.path.join(ROOT, "tests", "golden", "rechub_session.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d arrays, %d bytes)" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
