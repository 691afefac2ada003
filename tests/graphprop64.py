"""Graph propagation restated (helper of tests/test_graphprop_host.py and tests/test_gpu_graphprop.py, not a test).

``reference``: ``y = alpha (A * s) x + beta add`` with A dense in float64, and the gradients of ``sum(y * up)``:
``dx = alpha (A * s)^T up``, ``dadd = beta up``.  ``ref32``: the same in float32 on the CPU with plain torch ops, one
``index_add_`` over the edges -- the ``ref32`` of tests/fp32_bar.py.  ``mean_reference`` / ``mean_ref32``: ``mean_{k <= K} A^k x``
and the gradient ``mean_k (A^T)^k up``.

``make_graph(n_out, n_in)``: the edges of a test matrix whose rows have 0, 7, 8, 9 and min(29, n_in) edges (segment 8: one short
of a segment, a whole one, one past it, and three whole segments plus 5), further empty rows, rows of 1 .. 12 edges, one
duplicated edge, and column 0 read by every row that has edges (34 of 37) -- so that the transposed side, which the backward
walks, has a row of more than 29 edges whatever n_in is.  (A 37 x 23 matrix cannot hold a row of 29 distinct columns: its
longest row is the full one, 23 = two segments plus 7.)"""
import functools
import os

import numpy as np
import torch


@functools.lru_cache(maxsize=None)
def fixture():
    """tests/golden/graphprop.npz (recorded by tests/gen_golden_graphprop.py) as {name: tensor}."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "graphprop.npz")
    with np.load(path) as z:
        return {k: torch.from_numpy(z[k]) for k in z.files}


def group(prefix):
    """The arrays ``prefix.<key>`` of the fixture as {key: tensor}."""
    return {k[len(prefix) + 1:]: v for k, v in fixture().items() if k.startswith(prefix + ".")}


def fixture_graph(norm_adj, device="cpu", segment=None):
    fx = fixture()
    return norm_adj(7, 9, fx["inter.user"].to(device), fx["inter.item"].to(device), segment)


def run_module(module, prefix, device):
    """Loads ``prefix.p.*`` into ``module``, runs ``forward()`` -> (user, item), backpropagates the fixture's functional and
    returns ({"user", "item"}, {parameter: gradient})."""
    module.load_state_dict(group(prefix + ".p"), strict=True)
    module.to(device).train()
    u, i = module()
    up = group(prefix)
    ((u * up["up_user"].to(device)).sum() + (i * up["up_item"].to(device)).sum()).backward()
    return {"user": u.detach().cpu(), "item": i.detach().cpu()}, {k: p.grad.cpu() for k, p in module.named_parameters()}


def make_graph(n_out, n_in, seed=0):
    g = torch.Generator().manual_seed(100 + seed)
    degs = [0, 7, 8, 9, min(29, n_in), 0] + [int(d) for d in torch.randint(1, 13, (n_out - 8,), generator=g)] + [0, 3]
    assert len(degs) == n_out
    rows, cols = [], []
    for i, d in enumerate(degs):
        if d == 0:
            continue
        picked = [0] + (torch.randperm(n_in - 1, generator=g) + 1)[:d - 1].tolist()
        rows += [i] * len(picked)
        cols += picked
    rows.append(rows[5])                                                  # one repeated edge: coalescing sums it
    cols.append(cols[5])
    rows, cols = torch.tensor(rows), torch.tensor(cols)
    order = torch.randperm(rows.numel(), generator=g)                     # COO input in no particular order
    vals = torch.randn(rows.numel(), generator=g)
    return rows[order], cols[order], vals, (n_out, n_in)


def dense64(G):
    return G.to_sparse_coo().cpu().to_dense().double()


def edges(G):
    return G.edge_rows().cpu(), G.col.cpu().long(), G.val.cpu()


def reference(G, x, up, add=None, alpha=1.0, beta=1.0, scale=None):
    A = dense64(G)
    if scale is not None:
        r, c, _ = edges(G)
        S = torch.zeros_like(A)
        S[r, c] = scale.double().cpu()
        A = A * S
    y = alpha * (A @ x.double())
    out = {"y": y, "dx": alpha * (A.t() @ up.double())}
    if add is not None:
        out["y"] = y + beta * add.double()
        out["dadd"] = beta * up.double()
    return out


def _spmm32(r, c, w, x, n_out):
    return torch.zeros((n_out, x.shape[1]), dtype=torch.float32).index_add_(0, r, w.unsqueeze(1) * x[c])


def ref32(G, x, up, add=None, alpha=1.0, beta=1.0, scale=None):
    r, c, v = edges(G)
    w = v if scale is None else v * scale.float().cpu()
    x, up = x.float(), up.float()
    y = alpha * _spmm32(r, c, w, x, G.shape[0])
    out = {"y": y, "dx": alpha * _spmm32(c, r, w, up, G.shape[1])}
    if add is not None:
        out["y"] = y + beta * add.float()
        out["dadd"] = beta * up
    return out


def mean_reference(G, x, up, K):
    A = dense64(G)
    y, g, px, pg = x.double().clone(), up.double().clone(), x.double(), up.double()
    for _ in range(K):
        px, pg = A @ px, A.t() @ pg
        y, g = y + px, g + pg
    return {"y": y / (K + 1), "dx": g / (K + 1)}


def mean_ref32(G, x, up, K):
    r, c, v = edges(G)
    n = G.shape[0]
    ys, gs = [x.float()], [up.float()]
    for _ in range(K):
        ys.append(_spmm32(r, c, v, ys[-1], n))
        gs.append(_spmm32(c, r, v, gs[-1], n))
    return {"y": torch.stack(ys, 1).mean(1), "dx": torch.stack(gs, 1).mean(1)}
