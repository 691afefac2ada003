"""Generate tests/golden/rechub_multi_interest_sa.npz from the LIVE reference (dev container only; run from the repository
root):

    python tests/gen_golden_sa.py

ComirecSA (third_party/rechub/models/matching/comirec.py) and SINE (sine.py) at B = 16, L = 6, D = 8, K = 3; SINE with hidden
12, 5 concepts, 3 intentions, 1 head.  One item table shared by the history, the target and 3 negatives; histories of lengths
0..6 (id 0 = padding, at least two empty); parameters seeded randn * 0.3, embeddings * 0.5, so that every attention logit is
far below 32 (asserted), where the reference's fp32 ``+ -1e9 (1 - mask)`` leaves exactly -1e9 at a masked position.  Both
models make a discrete choice -- the argmax over interests in ComirecSA, the top-k over concepts in SINE -- and a 1e-6
difference on another device could flip an index whose scores are closer than that: the generator asserts that for every sample
the last chosen and the first rejected score are more than 1e-3 apart and draws another seed if not.  (One exception, by
construction: a history of no item or one item gives ComirecSA K identical interest vectors -- every column of A is 1 / L, or
one-hot on that item -- so its scores tie exactly, on every device, and ``argmax`` takes the first; the generator asserts that
these ties are exact.)  A seed is also refused when moving every parameter by one fp32 rounding moves any recorded value by
more than 1e-5: SINE's ``F.normalize(t, -1)`` is a p = -1 norm, which can magnify roundings a thousandfold, and a fixture drawn
there would pin one machine's summation order, not the model.  Groups: ``in`` (ids)
and per model ``p_*`` (state_dict), ``out_*`` (y and the mode="user" output) and ``g_*`` (parameter gradients of y.sum()).
Data only."""
import copy
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, L, D, K, N_NEG = 16, 6, 8, 3, 3
HIDDEN, N_CONCEPT = 12, 5
N_USERS, N_ITEMS = 11, 23
MIN_GAP, MAX_LOGIT = 1e-3, 32.0
MAX_SENSITIVITY = 1e-5                         # a tenth of the tests' 1e-4, for a move of one rounding


def features(mod):
    user = [mod.SparseFeature("user_id", vocab_size=N_USERS, embed_dim=D)]
    hist = [mod.SequenceFeature("hist_item_id", vocab_size=N_ITEMS, embed_dim=D, pooling="concat", shared_with="item_id")]
    item = [mod.SparseFeature("item_id", vocab_size=N_ITEMS, embed_dim=D)]
    neg = [mod.SequenceFeature("neg_items", vocab_size=N_ITEMS, embed_dim=D, pooling="concat", shared_with="item_id")]
    return user, hist, item, neg


def seed_params(model, g):
    with torch.no_grad():
        for name, p in model.named_parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (0.5 if "embed" in name else 0.3))


def comirec_margins(model, x):
    """(largest |attention logit|, smallest gap between the best and the second interest score)"""
    model.mode = None
    with torch.no_grad():
        hist = model.embedding(x, model.history_features).squeeze(1)
        sa = model.multi_interest_sa
        logits = torch.tanh(hist @ sa.W1) @ sa.W2
        user, item = model.user_tower(x), model.item_tower(x)
        score = torch.bmm(user, item[:, 0, :].unsqueeze(-1)).squeeze(-1)
        top = torch.topk(score, 2, dim=1).values
        tied = (x["hist_item_id"] > 0).sum(dim=1) <= 1              # A = 1 / L, or one-hot on the one item, in every column
        assert (score[tied] == score[tied][:, :1]).all()            # identical interests: an exact tie, the first index wins
    return logits.abs().max().item(), (top[:, 0] - top[:, 1])[~tied].min().item()


def sine_margins(model, x):
    """(largest |attention logit| of the three stages, smallest gap between the last chosen and the first rejected concept)"""
    with torch.no_grad():
        hist = x["hist_item_id"]
        x_u = model.item_embedding(hist) + model.position_embedding.weight.unsqueeze(0)
        m = (hist > 0).float().unsqueeze(-1)
        l1 = torch.tanh(x_u @ model.w_1) @ model.w_2
        z_u = torch.einsum("bse, bsh -> be", x_u, torch.softmax(l1 + -1.e9 * (1 - m), dim=1))
        s_u = z_u @ model.concept_embedding.weight.t()
        top = torch.topk(s_u, model.num_intention + 1).values
        gap = (top[:, model.num_intention - 1] - top[:, model.num_intention]).min().item()
        sel = torch.topk(s_u, model.num_intention)
        c_u = torch.sigmoid(sel.values).unsqueeze(-1) * model.concept_embedding(sel.indices)
        p_u = torch.softmax(torch.einsum("bse, bke -> bks", torch.nn.functional.normalize(x_u @ model.w_3, dim=-1),
                                         torch.nn.functional.normalize(c_u, p=2, dim=-1)), dim=1)
        l2 = torch.tanh(x_u @ model.w_k1) @ model.w_k2
        x_hat = torch.einsum("bks, bke -> bse", p_u, c_u)
        l3 = torch.tanh(x_hat @ model.w_4) @ model.w_5
    return max(l1.abs().max().item(), l2.abs().max().item(), l3.abs().max().item()), gap


def results(tag, model, x):
    """{"out_<tag>.user" / ".item" / ".y", "g_<tag>.<parameter>"}: what the fixture records of one model"""
    res = {}
    model.train()
    model.zero_grad()
    model.mode = "user"
    res["out_%s.user" % tag] = model(x).detach().numpy()
    model.mode = "item"
    res["out_%s.item" % tag] = model(x).detach().numpy()
    model.mode = None
    y = model(x)
    y.sum().backward()
    res["out_%s.y" % tag] = y.detach().numpy()
    for name, p in model.named_parameters():
        res["g_%s.%s" % (tag, name)] = (p.grad if p.grad is not None else torch.zeros_like(p)).clone().numpy()
    return res


def sensitivity(tag, model, x, seed):
    """Largest change of any recorded value when every parameter moves by about one fp32 rounding (relative 1e-7, random):
    what another machine's summation order does to the fixture.  SINE's ``F.normalize(t, -1)`` is the p = -1 norm, t times
    the sum of 1 / |t_i|, which magnifies roundings without bound when a component of t is near zero."""
    base = results(tag, model, x)
    moved = copy.deepcopy(model)
    g = torch.Generator().manual_seed(seed + 7)
    with torch.no_grad():
        for p in moved.parameters():
            p.mul_(1 + 1e-7 * torch.randn(p.shape, generator=g))
    other = results(tag, moved, x)
    return max(float(np.abs(base[k] - other[k]).max()) for k in base)


def record(out, tag, model, x):
    for k, v in model.state_dict().items():
        out["p_%s.%s" % (tag, k)] = v.detach().clone().numpy()
    out.update(results(tag, model, x))


def main():
    from oracle import ref_shim
    # the reference's vendored deepctr asks a package index for its latest version when imported; generation runs offline
    offline = types.ModuleType("requests")
    offline.get = lambda *a, **k: (_ for _ in ()).throw(OSError("offline"))
    sys.modules.setdefault("requests", offline)
    ref_shim.import_reference()
    import torch_rechub.basic.features as feats
    from recbox.third_party.rechub.models.matching.comirec import ComirecSA
    from recbox.third_party.rechub.models.matching.sine import SINE

    g = torch.Generator().manual_seed(20262)
    lengths = torch.tensor([0, 6, 1, 2, 3, 4, 5, 6, 0, 3, 6, 1, 5, 2, 4, 0])
    assert (lengths == 0).sum() >= 2
    hist = torch.randint(1, N_ITEMS, (B, L), generator=g)
    hist = hist * (torch.arange(L).unsqueeze(0) < lengths.unsqueeze(1))
    x = {"user_id": torch.randint(0, N_USERS, (B,), generator=g), "hist_item_id": hist,
         "item_id": torch.randint(1, N_ITEMS, (B,), generator=g), "neg_items": torch.randint(1, N_ITEMS, (B, N_NEG), generator=g)}
    out = {"in." + n: t.numpy() for n, t in x.items()}
    for tag in ("comirec_sa", "sine"):
        for seed in range(100, 200):
            torch.manual_seed(seed)                      # ComirecSA's forward draws (and overwrites) a torch.rand buffer
            if tag == "comirec_sa":
                model = ComirecSA(*features(feats), interest_num=K)
            else:
                model = SINE(["hist_item_id"], ["item_id"], ["neg_items"], N_ITEMS, D, HIDDEN, N_CONCEPT, K, L, num_heads=1)
            seed_params(model, torch.Generator().manual_seed(seed))
            big, gap = (comirec_margins if tag == "comirec_sa" else sine_margins)(model, x)
            if big < MAX_LOGIT / 4 and gap > MIN_GAP:
                torch.manual_seed(seed)
                moves = sensitivity(tag, model, x, seed)
                if moves < MAX_SENSITIVITY:
                    break
        else:
            raise RuntimeError("no seed with a safe margin for " + tag)
        assert big < MAX_LOGIT and gap > MIN_GAP
        print("%s: seed %d, largest |logit| %.3f, smallest decision gap %.2e, moves by %.1e under one rounding"
              % (tag, seed, big, gap, moves))
        torch.manual_seed(seed)
        record(out, tag, model, x)
        assert tuple(out["out_%s.y" % tag].shape) == ((B, D) if tag == "comirec_sa" else (B, 1 + N_NEG))
    assert np.abs(out["g_comirec_sa.multi_interest_sa.W3"]).max() == 0.0
    path = os.path.join(ROOT, "tests", "golden", "rechub_multi_interest_sa.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d arrays, %d bytes)" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
