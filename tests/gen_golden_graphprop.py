"""Generate tests/golden/graphprop.npz from the LIVE reference (dev container only; run from the repository root):

    python tests/gen_golden_graphprop.py

RecBole's LightGCN and NGCF (third_party/recbole/model/general_recommender/lightgcn.py, ngcf.py) and ``BiGNNLayer``
(model/layers.py): ``get_norm_adj_mat`` and ``forward`` called unbound on a stand-in module that carries what they read --
``n_users``, ``n_items``, ``interaction_matrix`` (scipy COO), ``user_embedding``, ``item_embedding``, ``n_layers`` /
``GNNlayers``, ``norm_adj_matrix``, ``eye_matrix``, ``node_dropout``, ``message_dropout`` -- because the models' constructors
want RecBole's config and dataset (as tests/gen_golden_srgnn.py does).  The parameters are drawn by the reference's
``xavier_uniform_initialization`` / ``xavier_normal_initialization`` under a seed.

The graph: 7 users x 9 items, 20 interactions of which one is repeated; user 5 and item 7 have none.  Arrays: ``inter.user``,
``inter.item``; ``adj.row``, ``adj.col``, ``adj.val`` (the ``norm_adj_matrix``, coalesced); per n_layers K in (1, 3)
``lgcn<K>.p.*`` (parameters), ``lgcn<K>.user`` / ``.item`` (``forward()``), ``lgcn<K>.up_user`` / ``.up_item`` (the seeded
linear functional) and ``lgcn<K>.g.*`` (its gradients); ``ngcf.p.*``, ``ngcf.user`` / ``.item`` (one forward at embedding
size 8, hidden sizes [8, 4], node_dropout = 0 and message_dropout = 0), ``ngcf.up_*``, ``ngcf.g.*``; ``bignn.p.*``, ``bignn.x``
[16, 8], ``bignn.out`` [16, 4] (one ``BiGNNLayer(8, 4)`` on the same matrix), ``bignn.up``, ``bignn.g.*`` and ``bignn.gx``.  Data only.

The reference package imports its vendored deepctr, which asks a package index for its latest version from a thread when
imported; generation runs offline, so stand-ins are registered first and no request is ever started (as in
tests/gen_golden_fignn.py)."""
import importlib
import os
import sys

import numpy as np
import scipy.sparse as sp
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

N_USERS, N_ITEMS = 7, 9
USERS = [0, 0, 0, 1, 1, 2, 2, 2, 2, 3, 3, 4, 6, 6, 6, 6, 6, 1, 2, 0]       # user 5 has no interaction
ITEMS = [0, 3, 8, 1, 3, 0, 2, 4, 6, 3, 5, 8, 0, 1, 2, 3, 4, 1, 5, 6]       # item 7 has none; (1, 1) is there twice


def _stand_in(kind):
    nn = torch.nn
    host = nn.Module()
    host.n_users, host.n_items, host.device = N_USERS, N_ITEMS, torch.device("cpu")
    host.interaction_matrix = sp.coo_matrix((np.ones(len(USERS), dtype=np.float32), (np.array(USERS), np.array(ITEMS))),
                                            shape=(N_USERS, N_ITEMS))
    return host


def _params(host, out, tag):
    params = dict(host.named_parameters())
    assert sorted(params) == sorted(host.state_dict())
    for k, v in params.items():
        out["%s.p.%s" % (tag, k)] = v.detach().numpy().copy()
    return params


def main():
    import gen_golden_autoint
    gen_golden_autoint._offline()
    import gen_golden_recbole
    gen_golden_recbole.recbole_layers()
    base = "recbox.third_party.recbole.model"
    lg = importlib.import_module(base + ".general_recommender.lightgcn")
    ng = importlib.import_module(base + ".general_recommender.ngcf")
    init = importlib.import_module(base + ".init")
    layers = importlib.import_module(base + ".layers")
    nn = torch.nn
    if not hasattr(sp.dok_matrix, "_update"):
        # the reference fills its dok matrix through a private method that newer scipy dropped: the same dict update
        sp.dok_matrix._update = lambda self, data: self._dict.update(data)
    out = {"inter.user": np.array(USERS, dtype=np.int64), "inter.item": np.array(ITEMS, dtype=np.int64)}

    host = _stand_in("lightgcn")
    adj = lg.LightGCN.get_norm_adj_mat(host).coalesce()
    adj2 = ng.NGCF.get_norm_adj_mat(host).coalesce()
    assert torch.equal(adj.indices(), adj2.indices()) and torch.equal(adj.values(), adj2.values())
    assert adj.values().dtype == torch.float32
    out.update({"adj.row": adj.indices()[0].numpy(), "adj.col": adj.indices()[1].numpy(), "adj.val": adj.values().numpy()})
    N = N_USERS + N_ITEMS

    for K in (1, 3):
        torch.manual_seed(700 + K)
        g = torch.Generator().manual_seed(300 + K)
        host = _stand_in("lightgcn")
        host.latent_dim, host.n_layers = 8, K
        host.user_embedding = nn.Embedding(N_USERS, 8)
        host.item_embedding = nn.Embedding(N_ITEMS, 8)
        host.norm_adj_matrix = adj
        host.get_ego_embeddings = lambda host=host: lg.LightGCN.get_ego_embeddings(host)
        host.apply(init.xavier_uniform_initialization)
        tag = "lgcn%d" % K
        params = _params(host, out, tag)
        u, i = lg.LightGCN.forward(host)
        up_u, up_i = torch.randn(N_USERS, 8, generator=g), torch.randn(N_ITEMS, 8, generator=g)
        ((u * up_u).sum() + (i * up_i).sum()).backward()
        out.update({tag + ".user": u.detach().numpy(), tag + ".item": i.detach().numpy(), tag + ".up_user": up_u.numpy(),
                    tag + ".up_item": up_i.numpy()})
        for k, v in params.items():
            out["%s.g.%s" % (tag, k)] = v.grad.numpy().copy()
        print("%s: |user| max %.3f" % (tag, float(u.detach().abs().max())))

    torch.manual_seed(811)
    g = torch.Generator().manual_seed(311)
    host = _stand_in("ngcf")
    host.node_dropout, host.message_dropout = 0.0, 0.0
    host.user_embedding = nn.Embedding(N_USERS, 8)
    host.item_embedding = nn.Embedding(N_ITEMS, 8)
    host.GNNlayers = nn.ModuleList([layers.BiGNNLayer(8, 8), layers.BiGNNLayer(8, 4)])
    host.norm_adj_matrix = adj
    host.eye_matrix = ng.NGCF.get_eye_mat(host)
    host.get_ego_embeddings = lambda: ng.NGCF.get_ego_embeddings(host)
    host.apply(init.xavier_normal_initialization)
    params = _params(host, out, "ngcf")
    u, i = ng.NGCF.forward(host)
    assert tuple(u.shape) == (N_USERS, 20)
    up_u, up_i = torch.randn(N_USERS, 20, generator=g), torch.randn(N_ITEMS, 20, generator=g)
    ((u * up_u).sum() + (i * up_i).sum()).backward()
    out.update({"ngcf.user": u.detach().numpy(), "ngcf.item": i.detach().numpy(), "ngcf.up_user": up_u.numpy(),
                "ngcf.up_item": up_i.numpy()})
    for k, v in params.items():
        out["ngcf.g.%s" % k] = v.grad.numpy().copy()

    torch.manual_seed(822)
    layer = layers.BiGNNLayer(8, 4)
    layer.apply(init.xavier_normal_initialization)
    with torch.no_grad():
        layer.linear.bias.normal_(0, 0.1, generator=g)
        layer.interActTransform.bias.normal_(0, 0.1, generator=g)
    x = torch.randn(N, 8, generator=g).requires_grad_()
    up = torch.randn(N, 4, generator=g)
    y = layer(adj, ng.NGCF.get_eye_mat(host), x)
    (y * up).sum().backward()
    params = _params(layer, out, "bignn")
    out.update({"bignn.x": x.detach().numpy(), "bignn.out": y.detach().numpy(), "bignn.up": up.numpy(), "bignn.gx": x.grad.numpy()})
    for k, v in params.items():
        out["bignn.g.%s" % k] = v.grad.numpy().copy()

    path = os.path.join(ROOT, "tests", "golden", "graphprop.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d arrays, %d bytes)" % (path, len(out), os.path.getsize(path)))
    assert os.path.getsize(path) < 256 * 1024


if __name__ == "__main__":
    main()
