"""Generate tests/golden/caser.npz from the LIVE reference (dev container only; run from the repository root):

    python tests/gen_golden_caser.py

RecBole's Caser (third_party/recbole/model/sequential_recommender/caser.py): ``Caser.forward`` called unbound on a stand-in
module that carries what it reads -- ``n_h``, ``n_v``, ``fc1_dim_v``, ``user_embedding`` and ``item_embedding``
(``nn.Embedding(padding_idx=0)``), ``conv_v``, ``conv_h``, ``fc1``, ``fc2``, ``dropout`` (p = 0), ``ac_conv``, ``ac_fc`` -- because
the model's constructor wants RecBole's config and dataset.  The parameters are drawn by the reference's ``_init_weights``
under a seed; the convolutions keep ``nn.Conv2d``'s own initialisation, as in the reference.  Two departures, so that the
fixture shows more than biases: the item rows are scaled up to deviation 2 / sqrt(D) (at 1 / D every ReLU sits on its bias) and
the two Linear biases are drawn with deviation 0.1 instead of 0.

Per case c at (B, L, D, n_h, n_v, n_items) = (37, 10, 16, 8, 4, 23), (19, 5, 8, 3, 0, 11) and (11, 7, 4, 0, 2, 6), with 9 users:
``in<c>`` (``user`` [B], ``seq`` [B, L] left-aligned sessions of 1 .. L clicks padded with 0, ``up`` [B, D]), ``p<c>`` (the
stand-in's state_dict, whose keys are the reference model's), ``out<c>`` (``conv`` [B, n_v D + n_h L], what the reference hands
to its dropout, and ``seq_output`` = forward(user, seq) [B, D]) and ``g<c>`` (the gradients of ``sum(seq_output * up)`` with
respect to every parameter).  With one branch empty the reference's forward ends in ``torch.cat([None, out_h], 1)``, which
raises; for the second and third case the generator drops the ``None`` from that one call and changes nothing else.  Data only.

The reference package imports its vendored deepctr, which asks a package index for its latest version from a thread when
imported; generation runs offline, so stand-ins for ``requests`` (whose ``get`` raises) and for that package are registered
before the reference is imported and no request is ever started (as in tests/gen_golden_fignn.py)."""
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = ((37, 10, 16, 8, 4, 23), (19, 5, 8, 3, 0, 11), (11, 7, 4, 0, 2, 6))
N_USERS = 9


def _stand_in(mod, n_items, L, D, n_h, n_v):
    nn = torch.nn
    host = nn.Module()
    host.n_h, host.n_v = n_h, n_v
    host.user_embedding = nn.Embedding(N_USERS, D, padding_idx=0)
    host.item_embedding = nn.Embedding(n_items, D, padding_idx=0)
    host.conv_v = nn.Conv2d(in_channels=1, out_channels=n_v, kernel_size=(L, 1))
    host.conv_h = nn.ModuleList([nn.Conv2d(in_channels=1, out_channels=n_h, kernel_size=(i + 1, D)) for i in range(L)])
    host.fc1_dim_v = n_v * D
    host.fc1 = nn.Linear(n_v * D + n_h * L, D)
    host.fc2 = nn.Linear(D + D, D)
    host.dropout = nn.Dropout(0.0)
    host.ac_conv = nn.ReLU()
    host.ac_fc = nn.ReLU()
    host.apply(lambda m: mod.Caser._init_weights(host, m))
    with torch.no_grad():                                                           # a bias of 0 would hide a missing one
        host.fc1.bias.normal_(0, 0.1)
        host.fc2.bias.normal_(0, 0.1)
        host.item_embedding.weight.mul_(float(D) ** 0.5 * 2)                        # deviation 1 / D leaves every ReLU on its bias
        host.item_embedding.weight[0].zero_()
    return host


def _forward(mod, host, user, seq):
    if host.n_h and host.n_v:
        return mod.Caser.forward(host, user, seq)
    cat = torch.cat
    torch.cat = lambda ts, *a, **k: cat([t for t in ts if t is not None], *a, **k)
    try:
        return mod.Caser.forward(host, user, seq)
    finally:
        torch.cat = cat


def record(c, dims, mod, out):
    B, L, D, n_h, n_v, n_items = dims
    torch.manual_seed(700 + c)
    g = torch.Generator().manual_seed(300 + c)
    host = _stand_in(mod, n_items, L, D, n_h, n_v)
    lengths = torch.randint(1, L + 1, (B,), generator=g)
    lengths[0], lengths[1] = L, 1                                                   # a full row and a single click
    seq = torch.randint(1, n_items, (B, L), generator=g) * (torch.arange(L).unsqueeze(0) < lengths.unsqueeze(1))
    user = torch.randint(1, N_USERS, (B,), generator=g)
    up = torch.randn(B, D, generator=g)
    seen = []
    hook = host.dropout.register_forward_pre_hook(lambda m, a: seen.append(a[0].detach().clone()))
    y = _forward(mod, host, user, seq)
    hook.remove()
    assert tuple(y.shape) == (B, D) and tuple(seen[0].shape) == (B, n_v * D + n_h * L)
    (y * up).sum().backward()
    out.update({"in%d.user" % c: user.numpy(), "in%d.seq" % c: seq.numpy(), "in%d.up" % c: up.numpy(),
                "out%d.conv" % c: seen[0].numpy(), "out%d.seq_output" % c: y.detach().numpy()})
    params = dict(host.named_parameters())
    assert sorted(params) == sorted(host.state_dict())
    for k, v in params.items():
        out["p%d.%s" % (c, k)] = v.detach().numpy()
        out["g%d.%s" % (c, k)] = (v.grad if v.grad is not None else torch.zeros_like(v)).numpy()
    print("case %d %s: |seq_output| max %.3f, live conv outputs %.2f" % (c, dims, float(y.detach().abs().max()),
                                                                       float((seen[0] != 0).float().mean())))


def main():
    import gen_golden_autoint
    gen_golden_autoint._offline()
    import gen_golden_recbole
    gen_golden_recbole.recbole_layers()
    mod = importlib.import_module("recbox.third_party.recbole.model.sequential_recommender.caser")
    out = {}
    for c, dims in enumerate(CASES):
        record(c, dims, mod, out)
    path = os.path.join(ROOT, "tests", "golden", "caser.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d arrays, %d bytes)" % (path, len(out), os.path.getsize(path)))
    assert os.path.getsize(path) < 512 * 1024


if __name__ == "__main__":
    main()
