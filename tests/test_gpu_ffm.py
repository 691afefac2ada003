"""Field-aware FM on the HIP path (csrc/rbx_ffm.hip: ops.ffm_cross, the DeepFFM / FatDeepFFM mirrors) against the
restatement of tests/ffm64.py on the CPU: the Hadamard forward bit for bit in fp32 (one multiply, nothing to round
differently), the summed forward and every gradient against float64 within the project's absolute 1e-4.  Every float64
comparison also runs the fp32 composition this op replaces (F.embedding into [B, F, F, D], the FFM mirror) on the GPU
through the same asserts, so an input on which fp32 itself misses the bar shows as that."""
import pytest
import torch

import ffm64
from conftest import Fixture, assert_close

pytestmark = pytest.mark.gpu
TOL = 1e-4
B = 37
SHAPES = [(2, 16), (3, 16), (5, 16), (26, 16), (39, 16), (5, 4), (5, 8), (5, 12), (5, 20), (5, 32), (5, 64), (5, 128),
          (64, 16), (8, 128)]


def _inputs(F, D, batch=B, seed=0, blocks=None, std=1.0):
    g = torch.Generator().manual_seed(1000 * F + D + seed)
    blocks = blocks if blocks is not None else [1 + (7 * i + 3 * F) % 50 for i in range(F)]      # 1 .. 50 blocks
    tables = [torch.randn(nb * F, D, generator=g) * std for nb in blocks]
    ids = [torch.randint(0, nb, (batch,), generator=g) for nb in blocks]
    return tables, ids


def _composition(tables, ids, reduce_sum):
    """The fp32 composition on the device of the tables: what the models run when the gate refuses."""
    from recbox_amd.rechub.basic.layers import FFM
    F = len(tables)
    off = torch.arange(F, device=tables[0].device)
    rows = [torch.nn.functional.embedding(x.long().reshape(-1, 1) * F + off, t) for t, x in zip(tables, ids)]
    out = FFM(F, reduce_sum=reduce_sum).to(tables[0].device)(torch.stack(rows, dim=1))
    return out.squeeze(-1) if reduce_sum else out


def _grads(fn, tables, ids, reduce_sum, r, device):
    ts = [t.detach().to(device).requires_grad_(True) for t in tables]
    out = fn(ts, [x.to(device) for x in ids], reduce_sum)
    out.backward(r.to(device=device, dtype=out.dtype))
    return out.detach(), [t.grad for t in ts]


def _fused(tables, ids, reduce_sum):
    from recbox_amd import ops
    return ops.ffm_cross(tables, ids, reduce_sum=reduce_sum)


@pytest.mark.parametrize("F,D", SHAPES)
def test_hadamard_forward_is_bit_exact(F, D):
    from recbox_amd import ops
    tables, ids = _inputs(F, D)
    assert ops.ffm_supported([t.cuda() for t in tables], [x.cuda() for x in ids])
    with torch.no_grad():
        got = ops.ffm_cross([t.cuda() for t in tables], [x.cuda() for x in ids])
    want = ffm64.cross(tables, ids)                        # fp32 on the CPU
    assert got.shape == (B, F * (F - 1) // 2, D)
    assert torch.equal(got.cpu(), want)


@pytest.mark.parametrize("reduce_sum", [False, True])
@pytest.mark.parametrize("F,D", SHAPES)
def test_sum_and_gradients_against_float64(F, D, reduce_sum):
    tables, ids = _inputs(F, D, seed=1)
    P = F * (F - 1) // 2
    g = torch.Generator().manual_seed(7)
    r = torch.randn((B, P) if reduce_sum else (B, P, D), generator=g, dtype=torch.float64)
    want, gwant = _grads(lambda t, x, rs: ffm64.cross(t, x, rs), [t.double() for t in tables], ids, reduce_sum, r, "cpu")
    for name, fn in (("composition", _composition), ("fused", _fused)):
        got, ggot = _grads(fn, tables, ids, reduce_sum, r, "cuda")
        assert_close(got, want, TOL, "%s out F=%d D=%d" % (name, F, D))
        for i, (a, b) in enumerate(zip(ggot, gwant)):
            assert_close(a, b, TOL, "%s dtable %d F=%d D=%d" % (name, i, F, D))


@pytest.mark.parametrize("batch", [6181, 1])
@pytest.mark.parametrize("reduce_sum", [False, True])
def test_multiplicity(batch, reduce_sum):
    """Vocabularies of 1 and 3 blocks: runs of thousands of equal keys (the reduce's fix-up passes).  The upstream gradient
    is scaled by 1 / sqrt(B) so the run sums stay O(1); the fp32 composition meets the bar on these exact inputs on the CPU
    (checked when the seed was fixed: worst gradient error 8.8e-06, at B = 6181 with reduce_sum)."""
    F, D = 5, 16
    tables, ids = _inputs(F, D, batch=batch, seed=2, blocks=[1, 3, 1, 3, 3])
    P = F * (F - 1) // 2
    g = torch.Generator().manual_seed(11)
    r = torch.randn((batch, P) if reduce_sum else (batch, P, D), generator=g, dtype=torch.float64) / batch ** 0.5
    want, gwant = _grads(lambda t, x, rs: ffm64.cross(t, x, rs), [t.double() for t in tables], ids, reduce_sum, r, "cpu")
    for name, fn in (("composition", _composition), ("fused", _fused)):
        got, ggot = _grads(fn, tables, ids, reduce_sum, r, "cuda")
        assert_close(got, want, TOL, name + " out")
        for i, (a, b) in enumerate(zip(ggot, gwant)):
            assert_close(a, b, TOL, "%s dtable %d B=%d" % (name, i, batch))


def test_diagonal_rows_and_untouched_blocks_get_exact_zeros():
    F, D = 5, 16
    tables, ids = _inputs(F, D, blocks=[50, 40, 30, 20, 10])
    ids = [x % 7 for x in ids]                              # blocks 7.. are never looked up
    r = torch.ones(B, F * (F - 1) // 2, D)
    _, grads = _grads(_fused, tables, ids, False, r, "cuda")
    for i, (gr, x) in enumerate(zip(grads, ids)):
        gb = gr.cpu().view(-1, F, D)
        assert (gb[:, i] == 0).all(), "diagonal rows of table %d" % i
        touched = torch.zeros(gb.shape[0], dtype=torch.bool)
        touched[x] = True
        assert (gb[~touched] == 0).all(), "untouched blocks of table %d" % i
        assert (gb[touched].abs().sum((1, 2)) > 0).all()


def test_backward_is_deterministic():
    F, D = 26, 16
    tables, ids = _inputs(F, D, batch=3000, seed=3, blocks=[1 + i % 4 for i in range(F)])
    r = torch.randn(3000, F * (F - 1) // 2, D, generator=torch.Generator().manual_seed(5))
    _, g1 = _grads(_fused, tables, ids, False, r, "cuda")
    _, g2 = _grads(_fused, tables, ids, False, r, "cuda")
    for a, b in zip(g1, g2):
        assert torch.equal(a, b)


def test_id_dtypes_and_strides_give_the_same_bits():
    F, D = 5, 16
    tables, ids = _inputs(F, D, seed=4)
    r = torch.randn(B, F * (F - 1) // 2, D, generator=torch.Generator().manual_seed(6))
    base_out, base_g = _grads(_fused, tables, ids, False, r, "cuda")
    batch = torch.zeros(B, 2 * F + 1, dtype=torch.float64)
    for i, x in enumerate(ids):
        batch[:, 2 * i + 1] = x.double()
    batch = batch.cuda()
    variants = {"int32": [x.int() for x in ids], "float32": [x.float() for x in ids], "float64": [x.double() for x in ids],
                "columns": [batch[:, 2 * i + 1] for i in range(F)]}
    for name, v in variants.items():
        out, gr = _grads(_fused, tables, v, False, r, "cuda")
        assert torch.equal(out, base_out), name
        for a, b in zip(gr, base_g):
            assert torch.equal(a, b), name


def test_out_of_range_id_raises_and_spares_the_other_samples():
    from recbox_amd import ops
    F, D = 3, 8
    tables, ids = _inputs(F, D, blocks=[4, 5, 6])
    tables = [torch.cat([t, torch.randn(1, D)]) for t in tables]         # vocab = blocks * F + 1: the tail row is no block
    good = ffm64.cross([t[:-1] for t in tables], ids)
    bad = [x.clone() for x in ids]
    bad[1][5] = 5                                                        # 5 * F + F > vocab
    bad[2][9] = -1
    dev_t, dev_i = [t.cuda() for t in tables], [x.cuda() for x in bad]
    with pytest.raises(IndexError):
        ops.ffm_cross(dev_t, dev_i)
    old = ops.config.check_ids
    ops.config.check_ids = False
    try:
        ops.check_deferred_ids()
        with torch.no_grad():
            out = ops.ffm_cross(dev_t, dev_i).cpu()
        with pytest.raises(IndexError):
            ops.check_deferred_ids()
    finally:
        ops.config.check_ids = old
    keep = torch.ones(B, dtype=torch.bool)
    keep[5] = keep[9] = False
    assert torch.equal(out[keep], good[keep])
    pairs = ffm64.pairs(F)
    for b, f in ((5, 1), (9, 2)):
        for p, (i, j) in enumerate(pairs):
            if f in (i, j):
                assert (out[b, p] == 0).all()
            else:
                assert torch.equal(out[b, p], good[b, p])


@pytest.mark.parametrize("case", ["D=6", "D=256", "F*D=1040", "padding_idx", "shared table"])
def test_refused_shapes_run_the_composition(case):
    """The gate says no, ops.ffm_cross raises NotImplementedError where it is called anyway, and a DeepFFM of that shape
    still computes the restatement's result (through F.embedding and the FFM mirror)."""
    from recbox_amd import ops
    from recbox_amd.rechub.basic.features import SparseFeature
    from recbox_amd.rechub.models.ranking import DeepFFM
    F, D, pad, shared = {"D=6": (4, 6, None, False), "D=256": (3, 256, None, False), "F*D=1040": (13, 80, None, False),
                         "padding_idx": (4, 8, 0, False), "shared table": (4, 8, None, True)}[case]
    vocabs = [3 + i for i in range(F)] if not shared else [5] * F
    names = ["C%d" % i for i in range(F)]
    linear = [SparseFeature("L" + n, vocab_size=v, embed_dim=1) for n, v in zip(names, vocabs)]
    cross = [SparseFeature(n, vocab_size=v * F, embed_dim=D, padding_idx=pad if i == 1 else None,
                           shared_with=names[0] if (shared and i == 2) else None)
             for i, (n, v) in enumerate(zip(names, vocabs))]
    torch.manual_seed(3)
    model = DeepFFM(linear, cross, D, {"dims": [16, 8], "dropout": 0.0, "activation": "relu"})
    with torch.no_grad():
        for name, p in model.named_parameters():
            p.copy_(torch.randn(p.shape) * (0.5 if "embed_dict" in name else 0.3))
    model.cuda().train()
    g = torch.Generator().manual_seed(9)
    x = {n: torch.randint(0, v, (16,), generator=g) for n, v in zip(names, vocabs)}
    x.update({"L" + n: x[n] for n in names})
    tables = model._ffm_tables()
    assert not ops.ffm_supported([t.weight for t in tables], [x[n].cuda() for n in names], model._ffm_padding())
    if case != "padding_idx":                                 # (a feature's padding_idx is a host-side fact; the C refusal of a
        #                                                       descriptor that carries one: test_ffm_host.py)
        with pytest.raises(NotImplementedError):
            ops.ffm_cross([t.weight for t in tables], [x[n].cuda() for n in names])
    sd = {k: (v.detach().cpu().double() if v.is_floating_point() else v.cpu()) for k, v in model.state_dict().items()}
    for i, n in enumerate(names):
        if cross[i].shared_with is not None:
            sd["ffm_embedding.embed_dict.%s.weight" % n] = sd["ffm_embedding.embed_dict.%s.weight" % cross[i].shared_with]
    want = ffm64.deepffm_forward(sd, x, ["L" + n for n in names], names)
    got = model({k: v.cuda() for k, v in x.items()})
    assert_close(got, want, TOL, case)


def _mirror(tag, pad=None):
    from recbox_amd.rechub.basic.features import SparseFeature
    from recbox_amd.rechub.models.ranking import DeepFFM, FatDeepFFM
    F, D, vocabs = 4, 8, [3, 5, 7, 11]
    names = ["C%d" % i for i in range(F)]
    linear = [SparseFeature(n, vocab_size=v, embed_dim=1) for n, v in zip(names, vocabs)]
    cross = [SparseFeature(n, vocab_size=v * F, embed_dim=D, padding_idx=pad if i == 1 else None)
             for i, (n, v) in enumerate(zip(names, vocabs))]
    mlp = {"dims": [16, 8], "dropout": 0.0, "activation": "relu"}
    return FatDeepFFM(linear, cross, D, 2, mlp) if tag == "fat" else DeepFFM(linear, cross, D, mlp)


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("tag", ["deep", "fat"])
def test_mirrors_match_the_reference_fixture(tag, fused):
    from recbox_amd import ops
    fx = Fixture("rechub_deepffm")
    model = _mirror(tag)
    model.load_state_dict(fx.tensors("p_" + tag), strict=True)
    model.cuda().train()
    x = fx.tensors("in", "cuda")
    old = ops.config.ffm_fused
    ops.config.ffm_fused = fused
    try:
        y = model(x)
        y.sum().backward()
    finally:
        ops.config.ffm_fused = old
    assert_close(y, fx["out_" + tag]["y"], TOL, "y")
    for name, p in model.named_parameters():
        got = p.grad if p.grad is not None else torch.zeros_like(p)
        assert_close(got, fx["g_" + tag][name], TOL, "grad " + name)


def test_padding_idx_feature_still_matches_the_fixture_outputs():
    """A cross feature with a padding_idx is refused by the gate; the composition gives the fixture's outputs (a padding_idx
    only takes that row's gradient away)."""
    fx = Fixture("rechub_deepffm")
    model = _mirror("deep", pad=0)
    model.load_state_dict(fx.tensors("p_deep"), strict=True)
    model.cuda().train()
    assert_close(model(fx.tensors("in", "cuda")), fx["out_deep"]["y"], TOL, "y")


def test_capture_and_replay_match_eager_bit_for_bit():
    from recbox_amd import ops
    F, D, batch = 5, 16, 300
    blocks = [2, 9, 30, 4, 17]
    tables, _ = _inputs(F, D, batch=batch, seed=5, blocks=blocks)
    g = torch.Generator().manual_seed(21)
    id_sets = [[torch.randint(0, nb, (batch,), generator=g) for nb in blocks] for _ in range(3)]
    r = torch.randn(batch, F * (F - 1) // 2, D, generator=g).cuda()
    ts = [t.cuda().requires_grad_(True) for t in tables]
    static = [x.cuda().clone() for x in id_sets[0]]
    old = ops.config.check_ids
    ops.config.check_ids = False                               # no host read inside a capture
    try:
        def step():
            out = ops.ffm_cross(ts, static)
            return out, torch.autograd.grad(out, ts, r)

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step()                                             # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            s_out, s_grads = step()
        for ids in id_sets[1:]:
            for dst, src in zip(static, ids):
                dst.copy_(src.cuda())
            graph.replay()
            torch.cuda.synchronize()
            got_out, got_g = s_out.clone(), [t.clone() for t in s_grads]
            e_out = ops.ffm_cross(ts, [x.cuda() for x in ids])
            e_g = torch.autograd.grad(e_out, ts, r)
            assert torch.equal(got_out, e_out)
            for a, b in zip(got_g, e_g):
                assert torch.equal(a, b)
        ops.check_deferred_ids()
    finally:
        ops.config.check_ids = old


def test_peak_memory_stays_below_the_gathered_block():
    """The point of the op.  B = 2048, F = 26, D = 16, 10 blocks per table: out plus its gradient are F(F-1)/F^2 = 0.96 of
    the [B, F, F, D] block, the sort workspace about 4/(F D) = 0.01 of it per key / value array plus the reduce's chunk
    summaries, tables and gradients are negligible: the rise of the peak over forward + backward stays below 1.5 blocks.
    The composition holds the block, its gradient and the two indexed operands: about 2.9 blocks -- asserted too, so that
    the cap cannot pass vacuously."""
    batch, F, D = 2048, 26, 16
    tables, ids = _inputs(F, D, batch=batch, seed=6, blocks=[10] * F)
    block = batch * F * F * D * 4

    def rise(fn):
        ts = [t.cuda().requires_grad_(True) for t in tables]
        xs = [x.cuda() for x in ids]
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = fn(ts, xs, False)
        out.backward(torch.ones_like(out))
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
        del out, ts
        return peak

    rise(_fused)                                               # (first call: plan, side stream)
    fused, comp = rise(_fused), rise(_composition)
    print("peak rise: fused %.2f blocks, composition %.2f blocks" % (fused / block, comp / block))
    assert fused < 1.5 * block, fused / block
    assert comp > 1.5 * block, comp / block
