"""Graph propagation, the host side (no GPU): ops.PropGraph against scipy.sparse, its task list at the segment edges,
``norm_adj`` bit-equal to the recorded reference, the composition ops against float64 under the factor-4 bar of
tests/fp32_bar.py, the mirrors against tests/golden/graphprop.npz at 1e-4 (every parameter gradient included), the
``state_dict`` key sets and the refusals.  (No C-ABI symbols and no aliasing refusal: the propagation kernel is not in the
tree, DESIGN.md.)"""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import fp32_bar
import graphprop64 as gp


def _scipy_csr(r, c, v, shape):
    m = sp.coo_matrix((v.double().numpy(), (r.numpy(), c.numpy())), shape=shape).tocsr()
    m.sum_duplicates()
    m.sort_indices()
    return m


@pytest.mark.parametrize("shape", [(37, 37), (37, 23)])
def test_csr_transpose_and_t_perm_against_scipy(shape):
    from recbox_amd import ops
    r, c, v, _ = gp.make_graph(*shape)
    G = ops.PropGraph.from_coo(r, c, v, shape, segment=8)
    m = _scipy_csr(r, c, v, shape)
    assert m.nnz == G.nnz == r.numel() - 1                               # the repeated edge was summed
    assert G.row_ptr.dtype == torch.int64 and G.col.dtype == torch.int32 and G.val.dtype == torch.float32
    assert np.array_equal(G.row_ptr.numpy(), m.indptr) and np.array_equal(G.col.numpy(), m.indices)
    assert np.abs(G.val.numpy() - m.data).max() <= 1e-6
    t = m.T.tocsr()
    t.sort_indices()
    assert np.array_equal(G.t_row_ptr.numpy(), t.indptr) and np.array_equal(G.t_col.numpy(), t.indices)
    assert G.t_perm.dtype == torch.int32 and torch.equal(G.val[G.t_perm.long()], G.t_val)
    assert torch.equal(G.edge_rows()[G.t_perm.long()], G.t_col.long())   # t_perm: each edge of A^T in A's edge order
    T = G.t()
    assert T.shape == (shape[1], shape[0]) and T.col.data_ptr() == G.t_col.data_ptr() and T.t().col.data_ptr() == G.col.data_ptr()
    assert torch.equal(T.val[T.t_perm.long()], G.val)
    coo = G.to_sparse_coo()
    assert coo.is_coalesced() and np.abs(coo.to_dense().double().numpy() - m.toarray()).max() <= 1e-6
    dup = ops.PropGraph.from_coo(torch.tensor([1, 1, 0, 1]), torch.tensor([2, 2, 0, 2]), torch.tensor([1.0, 2.0, 5.0, 4.0]), (3, 4))
    assert dup.col.tolist() == [0, 2] and dup.val.tolist() == [5.0, 7.0] and dup.row_ptr.tolist() == [0, 1, 2, 2]


@pytest.mark.parametrize("segment", [1, 2, 8])
def test_task_list_at_the_segment_edges(segment):
    """Rows of segment - 1, segment, segment + 1 and 3 segment + 5 edges and empty rows: every edge in exactly one task, a row
    of at most ``segment`` edges one direct task, a longer one ceil(len / segment) partial tasks in order plus one record."""
    from recbox_amd import ops
    lens = [0, segment - 1, segment, segment + 1, 0, 3 * segment + 5, 1, 0]
    rows = torch.tensor([i for i, n in enumerate(lens) for _ in range(n)])
    cols = torch.tensor([j for n in lens for j in range(n)])
    G = ops.PropGraph.from_coo(rows, cols, torch.ones(rows.numel()), (len(lens), 40), segment=segment)
    s = G._side
    start, length, dst = s.task_start.tolist(), s.task_len.tolist(), s.task_dst.tolist()
    assert s.task_start.dtype == torch.int64 and s.task_len.dtype == torch.int32 and s.task_dst.dtype == torch.int32
    want_tasks = sum(max(1, -(-n // segment)) for n in lens)
    assert s.n_tasks == want_tasks == len(start)
    ptr = G.row_ptr.tolist()
    t, slot, fin_row, fin_ptr = 0, 0, [], [0]
    for i, n in enumerate(lens):
        k = max(1, -(-n // segment))
        for j in range(k):
            assert start[t] == ptr[i] + j * segment and length[t] == min(segment, max(n - j * segment, 0))
            if k == 1:
                assert dst[t] == i
            else:
                assert dst[t] == -(slot + 1)
                slot += 1
            t += 1
        if k > 1:
            fin_row.append(i)
            fin_ptr.append(slot)
    assert s.n_partials == slot and s.n_fin == len(fin_row)
    assert s.fin_row.tolist() == fin_row and s.fin_ptr.tolist() == fin_ptr
    assert max(length) <= segment and sum(length) == G.nnz


def test_norm_adj_is_bit_equal_to_the_reference():
    from recbox_amd import recbole
    fx = gp.fixture()
    G = gp.fixture_graph(recbole.norm_adj)
    coo = G.to_sparse_coo()
    assert G.shape == (16, 16)
    assert torch.equal(coo.indices()[0], fx["adj.row"]) and torch.equal(coo.indices()[1], fx["adj.col"])
    assert torch.equal(coo.values(), fx["adj.val"])
    deg = G.row_ptr[1:] - G.row_ptr[:-1]
    assert deg[5] == 0 and deg[7 + 7] == 0 and G.nnz == 2 * 19           # a user and an item without edges; 20 - 1 pairs


@pytest.mark.parametrize("shape", [(37, 37), (37, 23)])
def test_composition_against_float64(shape):
    from recbox_amd import ops
    r, c, v, _ = gp.make_graph(*shape)
    G = ops.PropGraph.from_coo(r, c, v, shape, segment=8)
    g = torch.Generator().manual_seed(5)
    x, add, up = torch.randn(shape[1], 12, generator=g), torch.randn(shape[0], 12, generator=g), torch.randn(shape[0], 12, generator=g)
    scale = torch.rand(G.nnz, generator=g)
    scale[::4] = 0.0
    xs = (x[:9].clone().requires_grad_(), x[9:].clone().requires_grad_())
    a = add.clone().requires_grad_()
    y = ops.graph_prop(G, xs, a, 0.5, -2.0, scale)                        # CPU tensors: graph_prop_torch
    grads = torch.autograd.grad((y * up).sum(), xs + (a,))
    got = {"y": y.detach(), "dx": torch.cat(grads[:2], 0), "dadd": grads[2]}
    want = gp.reference(G, x, up, add, 0.5, -2.0, scale)
    r32 = gp.ref32(G, x, up, add, 0.5, -2.0, scale)
    for n in want:
        fp32_bar.assert_bar("%s %s" % (n, shape), got[n], want[n], r32[n])
    assert ops.graph_prop_torch(G, x.double()).dtype == torch.float64


@pytest.mark.parametrize("K", [0, 1, 3])
def test_mean_composition_against_float64(K):
    from recbox_amd import ops
    r, c, v, shape = gp.make_graph(37, 37)
    G = ops.PropGraph.from_coo(r, c, v, shape, segment=8)
    g = torch.Generator().manual_seed(6)
    x, up = torch.randn(37, 12, generator=g), torch.randn(37, 12, generator=g)
    xs = (x[:15].clone().requires_grad_(), x[15:].clone().requires_grad_())
    y = ops.graph_prop_mean(G, xs, K)
    y = torch.cat(y, 0) if isinstance(y, tuple) else y
    dx = torch.cat(torch.autograd.grad((y * up).sum(), xs), 0)
    want, r32 = gp.mean_reference(G, x, up, K), gp.mean_ref32(G, x, up, K)
    fp32_bar.assert_bar("y K%d" % K, y, want["y"], r32["y"])
    fp32_bar.assert_bar("dx K%d" % K, dx, want["dx"], r32["dx"])
    layers = ops.graph_prop_mean(G, x, K, layers=True)
    assert len(layers) == K + 1 and torch.equal(layers[0], x)


def _close(got, want, what):
    assert sorted(got) == sorted(want), what
    for n in want:
        assert tuple(got[n].shape) == tuple(want[n].shape) and (got[n] - want[n]).abs().max() <= 1e-4, "%s %s" % (what, n)


@pytest.mark.parametrize("K", [1, 3])
def test_lightgcn_encoder_against_the_fixture(K):
    from recbox_amd import recbole
    enc = recbole.LightGCNEncoder(7, 9, 8, K, gp.fixture_graph(recbole.norm_adj))
    assert sorted(enc.state_dict()) == ["item_embedding.weight", "user_embedding.weight"]
    out, grads = gp.run_module(enc, "lgcn%d" % K, "cpu")
    want = gp.group("lgcn%d" % K)
    _close(out, {"user": want["user"], "item": want["item"]}, "lightgcn forward")
    _close(grads, gp.group("lgcn%d.g" % K), "lightgcn gradients")


def test_ngcf_bignn_and_losses_against_the_fixture():
    from recbox_amd import recbole
    graph = gp.fixture_graph(recbole.norm_adj)
    enc = recbole.NGCFEncoder(7, 9, 8, [8, 4], graph, node_dropout=0.0, message_dropout=0.0)
    assert sorted(enc.state_dict()) == sorted(gp.group("ngcf.p"))
    assert "GNNlayers.1.interActTransform.bias" in enc.state_dict() and float(enc.GNNlayers[0].linear.bias.detach().abs().max()) == 0.0
    out, grads = gp.run_module(enc, "ngcf", "cpu")
    want = gp.group("ngcf")
    _close(out, {"user": want["user"], "item": want["item"]}, "ngcf forward")
    _close(grads, gp.group("ngcf.g"), "ngcf gradients")
    b = gp.group("bignn")
    layer = recbole.BiGNNLayer(8, 4)
    assert sorted(layer.state_dict()) == ["interActTransform.bias", "interActTransform.weight", "linear.bias", "linear.weight"]
    layer.load_state_dict(gp.group("bignn.p"), strict=True)
    x = b["x"].clone().requires_grad_()
    y = layer(graph, x)
    (y * b["up"]).sum().backward()
    _close({"out": y.detach(), "gx": x.grad}, {"out": b["out"], "gx": b["gx"]}, "bignn")
    _close({n: p.grad for n, p in layer.named_parameters()}, gp.group("bignn.g"), "bignn gradients")
    g = torch.Generator().manual_seed(1)
    pos, neg, e = torch.randn(11, generator=g), torch.randn(11, generator=g), torch.randn(5, 4, generator=g)
    assert torch.allclose(recbole.BPRLoss()(pos, neg), -torch.log(1e-10 + torch.sigmoid(pos - neg)).mean())
    assert torch.allclose(recbole.EmbLoss()(e, e[:3]), (e.norm() + e[:3].norm()).reshape(1) / 3)
    assert torch.allclose(recbole.EmbLoss()(e, require_pow=True), e.pow(2).sum().reshape(1) / 5 / 2)


def test_rechub_lightgcn_is_registered_and_scores_on_the_cpu():
    from recbox_amd import compat, recbole
    from recbox_amd.rechub.basic.features import SparseFeature
    from recbox_amd.rechub.models.matching import LightGCN
    assert "LightGCN" in compat.alias_also()["torch_rechub.models.matching"]
    model = LightGCN(SparseFeature("user_id", 7, 8), SparseFeature("item_id", 9, 8), gp.fixture_graph(recbole.norm_adj), n_layers=3)
    assert sorted(model.state_dict()) == ["encoder.item_embedding.weight", "encoder.user_embedding.weight"]
    model.encoder.load_state_dict(gp.group("lgcn3.p"), strict=True)
    want = gp.group("lgcn3")
    users, items = torch.tensor([0, 5, 6]), torch.tensor([[0, 7], [1, 8], [4, 3]])
    scores = model({"user_id": users, "item_id": items})
    assert (scores - (want["user"][users].unsqueeze(1) * want["item"][items]).sum(-1)).abs().max() <= 1e-4


def test_refusals():
    from recbox_amd import ops
    with pytest.raises(ValueError):
        ops.PropGraph.from_coo(torch.tensor([0]), torch.tensor([0]), torch.ones(1), (2 ** 31, 4))
    with pytest.raises(ValueError):
        ops.PropGraph.from_coo(torch.tensor([0]), torch.tensor([0]), torch.ones(1), (4, 2 ** 31))
    with pytest.raises(ValueError):
        ops.PropGraph.from_coo(torch.tensor([0]), torch.tensor([4]), torch.ones(1), (4, 4))
    G = ops.PropGraph.from_coo(torch.tensor([0, 1]), torch.tensor([1, 0]), torch.ones(2), (2, 2))
    with pytest.raises(RuntimeError):
        ops.graph_prop(G, torch.zeros(2, 4), edge_scale=torch.ones(2, requires_grad=True))
    with pytest.raises(RuntimeError):
        ops.graph_prop(G, torch.zeros(3, 4))
    with pytest.raises(RuntimeError):
        ops.graph_prop_mean(ops.PropGraph.from_coo(torch.tensor([0]), torch.tensor([1]), torch.ones(1), (2, 3)), torch.zeros(3, 4), 1)
