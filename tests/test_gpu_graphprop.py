"""Graph propagation on the GPU: ops.graph_prop / ops.graph_prop_mean (the torch.sparse.mm composition on CUDA tensors; the
propagation kernel is not in the tree) against the float64 restatement of tests/graphprop64.py under
tests/fp32_bar.py's bar with factor 4, and the LightGCN / NGCF mirrors -- whose Linears, dropout, normalisation and scores are
the library's kernels on CUDA tensors -- against tests/golden/graphprop.npz (recorded from the live reference) at 1e-4.

The graphs (graphprop64.make_graph) hold empty rows and rows of 7, 8, 9 and 29 edges (37 x 37; a 37 x 23 matrix has no row of
29 distinct columns: its longest is the full one, 23); column 0 is read by every row that has edges."""
import functools

import pytest
import torch

import fp32_bar
import graphprop64 as gp

pytestmark = pytest.mark.gpu
SHAPES = {"square": (37, 37), "rect": (37, 23)}


@functools.lru_cache(maxsize=None)
def _graphs(name):
    from recbox_amd import ops
    r, c, v, shape = gp.make_graph(*SHAPES[name])
    return ops.PropGraph.from_coo(r, c, v, shape, segment=8), ops.PropGraph.from_coo(r.cuda(), c.cuda(), v.cuda(), shape, segment=8)


@functools.lru_cache(maxsize=None)
def _data(name, D, seed=0):
    n_out, n_in = SHAPES[name]
    G, _ = _graphs(name)
    g = torch.Generator().manual_seed(7 + seed)
    scale = torch.rand(G.nnz, generator=g) + 0.5
    scale[::5] = 0.0
    return {"x": torch.randn(n_in, D, generator=g), "add": torch.randn(n_out, D, generator=g),
            "up": torch.randn(n_out, D, generator=g), "scale": scale}


def test_the_device_graph_is_the_host_graph():
    for name, longest in (("square", 29), ("rect", 23)):
        G, Gc = _graphs(name)
        deg = (G.row_ptr[1:] - G.row_ptr[:-1]).tolist()
        assert {0, 7, 8, 9, longest} <= set(deg)
        for a in ("row_ptr", "col", "val", "t_row_ptr", "t_col", "t_val", "t_perm"):
            assert getattr(Gc, a).is_cuda and torch.equal(getattr(Gc, a).cpu(), getattr(G, a)), a
        for a in ("task_start", "task_len", "task_dst", "fin_row", "fin_ptr"):
            assert torch.equal(getattr(Gc._side, a).cpu(), getattr(G._side, a)) and torch.equal(getattr(Gc._tside, a).cpu(), getattr(G._tside, a))


@pytest.mark.parametrize("name", ["square", "rect"])
@pytest.mark.parametrize("D", [6, 64])
def test_graph_prop_against_float64(D, name):
    from recbox_amd import ops
    G, Gc = _graphs(name)
    d = _data(name, D)
    for form in (dict(), dict(add=True, alpha=0.75, beta=-1.5), dict(add=True, alpha=2.0, beta=0.5, scale=True)):
        xs = [d["x"][:11].cuda().requires_grad_(), d["x"][11:].cuda().requires_grad_()]
        add = d["add"].cuda().requires_grad_() if form.get("add") else None
        y = ops.graph_prop(Gc, tuple(xs), add, form.get("alpha", 1.0), form.get("beta", 1.0), d["scale"].cuda() if form.get("scale") else None)
        grads = torch.autograd.grad((y * d["up"].cuda()).sum(), xs + ([add] if add is not None else []))
        got = {"y": y.detach(), "dx": torch.cat(grads[:2], 0)}
        if add is not None:
            got["dadd"] = grads[2]
        args = (d["add"] if form.get("add") else None, form.get("alpha", 1.0), form.get("beta", 1.0), d["scale"] if form.get("scale") else None)
        want, r32 = gp.reference(G, d["x"], d["up"], *args), gp.ref32(G, d["x"], d["up"], *args)
        assert sorted(got) == sorted(want)
        for n in want:
            fp32_bar.assert_bar("%s %s D%d %s" % (n, name, D, sorted(form)), got[n], want[n], r32[n])


@pytest.mark.parametrize("K", [0, 1, 3])
def test_mean_propagation_against_float64(K):
    from recbox_amd import ops
    G, Gc = _graphs("square")
    d = _data("square", 16, seed=1)
    xs = [d["x"][:15].cuda().requires_grad_(), d["x"][15:].cuda().requires_grad_()]
    y = ops.graph_prop_mean(Gc, tuple(xs), K)
    y = torch.cat(y, 0) if isinstance(y, tuple) else y
    dx = torch.cat(torch.autograd.grad((y * d["up"].cuda()).sum(), xs), 0)
    want, r32 = gp.mean_reference(G, d["x"], d["up"], K), gp.mean_ref32(G, d["x"], d["up"], K)
    fp32_bar.assert_bar("y mean K%d" % K, y, want["y"], r32["y"])
    fp32_bar.assert_bar("dx mean K%d" % K, dx, want["dx"], r32["dx"])
    assert len(ops.graph_prop_mean(Gc, d["x"].cuda(), K, layers=True)) == K + 1


@pytest.mark.parametrize("K", [1, 3])
def test_lightgcn_encoder_against_the_reference_fixture(K):
    from recbox_amd import recbole
    enc = recbole.LightGCNEncoder(7, 9, 8, K, gp.fixture_graph(recbole.norm_adj))
    out, grads = gp.run_module(enc, "lgcn%d" % K, "cuda")
    want, gwant = gp.group("lgcn%d" % K), gp.group("lgcn%d.g" % K)
    for n in ("user", "item"):
        assert (out[n] - want[n]).abs().max() <= 1e-4, n
    assert sorted(grads) == sorted(gwant)
    for n in gwant:
        assert (grads[n] - gwant[n]).abs().max() <= 1e-4, n


def test_rechub_lightgcn_against_the_reference_fixture():
    from recbox_amd import recbole
    from recbox_amd.rechub.basic.features import SparseFeature
    from recbox_amd.rechub.models.matching import LightGCN
    model = LightGCN(SparseFeature("user_id", 7, 8), SparseFeature("item_id", 9, 8), gp.fixture_graph(recbole.norm_adj), n_layers=3)
    model.encoder.load_state_dict(gp.group("lgcn3.p"), strict=True)
    model.cuda()
    want = gp.group("lgcn3")
    users = torch.tensor([0, 5, 6, 3]).cuda()
    items = torch.tensor([[0, 7, 2], [1, 1, 8], [4, 3, 0], [5, 6, 7]]).cuda()
    scores = model({"user_id": users, "item_id": items})
    ref = (want["user"][users.cpu()].unsqueeze(1) * want["item"][items.cpu()]).sum(-1)
    assert scores.shape == (4, 3) and (scores.cpu() - ref).abs().max() <= 1e-4
    scores.sum().backward()
    assert model.encoder.user_embedding.weight.grad is not None
    model.mode = "user"
    assert (model({"user_id": users}).cpu() - want["user"][users.cpu()]).abs().max() <= 1e-4
    model.mode = "item"
    assert (model({"item_id": items[:, 0]}).cpu() - want["item"][items[:, 0].cpu()]).abs().max() <= 1e-4
    model.eval()
    full = model.encoder.full_sort_predict(users)
    assert (full.cpu() - want["user"][users.cpu()] @ want["item"].t()).abs().max() <= 1e-4


def test_ngcf_encoder_and_bignn_layer_against_the_reference_fixture():
    from recbox_amd import recbole
    graph = gp.fixture_graph(recbole.norm_adj)
    enc = recbole.NGCFEncoder(7, 9, 8, [8, 4], graph, node_dropout=0.0, message_dropout=0.0)
    out, grads = gp.run_module(enc, "ngcf", "cuda")
    want, gwant = gp.group("ngcf"), gp.group("ngcf.g")
    for n in ("user", "item"):
        assert (out[n] - want[n]).abs().max() <= 1e-4, n
    assert sorted(grads) == sorted(gwant)
    for n in gwant:
        assert (grads[n] - gwant[n]).abs().max() <= 1e-4, n
    b = gp.group("bignn")
    layer = recbole.BiGNNLayer(8, 4)
    layer.load_state_dict(gp.group("bignn.p"), strict=True)
    layer.cuda()
    x = b["x"].cuda().requires_grad_()
    y = layer(graph.to("cuda"), x)
    (y * b["up"].cuda()).sum().backward()
    assert (y.detach().cpu() - b["out"]).abs().max() <= 1e-4 and (x.grad.cpu() - b["gx"]).abs().max() <= 1e-4
    for n, p in layer.named_parameters():
        assert (p.grad.cpu() - gp.group("bignn.g")[n]).abs().max() <= 1e-4, n
    # node dropout: a scale of 0 or 1 / keep per edge, drawn once per forward
    enc.node_dropout = 0.25
    s = enc.edge_scale()
    assert s.shape == (graph.nnz,) and set(s.unique().tolist()) <= {0.0, float(torch.tensor(1.0 / 0.75))}
    enc.train()
    assert enc()[0].shape == (7, 20)
