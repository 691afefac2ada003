"""The generic embedding lookup (rbx_embed_fwd / rbx_embed_sort / rbx_embed_bwd through recbox_amd._embed_host.Plan, and
DotPolicy's share of the sorted reduce through ops.gather_dot) against the float64 restatement of oracle/embed64.py at
every lane-group form, with the per-element bound |got - want| <= C eps32 A + tiny (backward: C = C_BOUND = 64; forward:
max(64, seq_len + 2) for pooled columns, equality for copies).  Rows with A = 0 -- never looked up, padding rows, rows
that only masked ids name -- must be exactly zero.

Which instantiation a dim selects (units = D / 4 when every field of the launch is 16-byte aligned and D % 4 == 0, else
D; G = min(64, next power of two >= units), NV = units' power of two / 64 beyond that):
  forward   one-id, numeric: embed_fwd_kernel<G, NV, VEC>; histories: embed_seq_kernel<SG, SG / G, NV, VEC> with
            SG = 16 (G <= 8), 32 (G = 16), 64 (G = 32, 64)
  backward  dispatch_reduce: segment_reduce_kernel / segment_fixup_short_kernel / segment_fixup_long_kernel<Policy, G, NV, VEC>
            from the plan's widest row; one field that is not 16-byte aligned makes the whole call scalar
  D                       fwd <G, NV, VEC>   seq <SG, R, NV, VEC>   bwd <G, NV, VEC>
  1                       <1, 1, false>      <16, 16, 1, false>     <1, 1, false>
  2                       <2, 1, false>      <16, 8, 1, false>      <2, 1, false>
  3                       <4, 1, false>      <16, 4, 1, false>      <4, 1, false>
  7                       <8, 1, false>      <16, 2, 1, false>      <8, 1, false>
  10                      <16, 1, false>     <32, 2, 1, false>      <16, 1, false>
  17                      <32, 1, false>     <64, 2, 1, false>      <32, 1, false>
  33, 63                  <64, 1, false>     <64, 1, 1, false>      <64, 1, false>
  65, 127                 <64, 2, false>     <64, 1, 2, false>      <64, 2, false>
  129, 255                <64, 4, false>     <64, 1, 4, false>      <64, 4, false>
  257                     refused (RBX_ERR_UNSUPPORTED)
  4                       <1, 1, true>       <16, 16, 1, true>      <1, 1, true>
  8                       <2, 1, true>       <16, 8, 1, true>       <2, 1, true>
  12, 16                  <4, 1, true>       <16, 4, 1, true>       <4, 1, true>
  20, 32                  <8, 1, true>       <16, 2, 1, true>       <8, 1, true>
  36, 64                  <16, 1, true>      <32, 2, 1, true>       <16, 1, true>
  68, 100, 128            <32, 1, true>      <64, 2, 1, true>       <32, 1, true>
  132, 192, 252, 256      <64, 1, true>      <64, 1, 1, true>       <64, 1, true>
  260, 384, 512           <64, 2, true>      <64, 1, 2, true>       <64, 2, true>
  516, 1000, 1024         <64, 4, true>      <64, 1, 4, true>       <64, 4, true>
  1028                    refused (RBX_ERR_UNSUPPORTED)
The hot-row cases at D = 132 and 256 are the ones the fused FM body's 64-lane finding pointed at: they pass here for
GenericPolicy and DotPolicy, which clears the three shared kernels (see test_gpu_fm_dims.py's header)."""
import pytest
import torch

from conftest import _note
from oracle.embed64 import C_BOUND, Table, bound_ratio, embed64, forward_ratio
from test_embed64_restatement import (grid_case, history, hot_row_batch, hot_row_dy, lookups64, magnitudes, make_table, spec,
                                      widths)

pytestmark = pytest.mark.gpu

VEC_NV1 = [4, 8, 12, 16, 20, 32, 36, 64, 68, 100, 128, 132, 192, 252, 256]
VEC_NVN = [260, 384, 512, 516, 1000, 1024]
SCALAR_NV1 = [1, 2, 3, 7, 10, 17, 33, 63]
SCALAR_NVN = [65, 127, 129, 255]
BEYOND = [16, 128, 132, 256, 512]
_POOL = {"NONE": 0, "SUM": 1, "MEAN_VALUE": 2, "MEAN_ID": 3, "SUM_ID": 4, "CONCAT": 5}
COMPACT_ABOVE = 4096            # tables with more rows are restated on the rows the batch names only


def form(D, vec=None):
    """"vector NV1" ...: the lane-group form a plan whose widest row has D floats runs in."""
    vec = (D % 4 == 0) if vec is None else vec
    units = D // 4 if vec else D
    return "%s NV%d" % ("vector" if vec else "scalar", 1 if units <= 64 else (2 if units <= 128 else 4))


class Device(object):
    """The modules (one per table key) and the host plan of a case on the GPU."""

    def __init__(self, specs, tables, offsets=None, width=None, modules=None):
        from recbox_amd import _embed_host as host
        from recbox_amd._lib import FIELD_CATEGORICAL, FIELD_DENSE, FIELD_NUMERIC
        self.specs, self.modules = specs, dict(modules or {})
        for key, (w, pad) in tables.items():
            if key in self.modules:                      # another plan's module: one parameter for both
                continue
            if w.dim() == 1:
                m = torch.nn.Linear(1, w.shape[0], bias=False)
                m.weight.data.copy_(w.view(-1, 1))
            else:
                m = torch.nn.Embedding(w.shape[0], w.shape[1], padding_idx=pad)
                m.weight.data.copy_(w)
            self.modules[key] = m.cuda()
        kinds = {"categorical": FIELD_CATEGORICAL, "numeric": FIELD_NUMERIC, "dense": FIELD_DENSE}
        lookups = []
        for s in specs:
            m = self.modules[s["table"]] if s["table"] else None
            D = 1 if m is None else tables[s["table"]][0].shape[-1]
            lookups.append(host.Lookup(s["name"], kinds[s["kind"]], m, D, pool=_POOL[s["pool"]], seq_len=s["L"],
                                       mask_id=s["mask_id"], eps=s["eps"]))
        self.plan = host.Plan(lookups, offsets=offsets, width=width)

    def inputs(self, cols, id_dtype):
        out = []
        for s in self.specs:
            c = cols[s["name"]]
            if s["kind"] == "categorical":
                c = c.to(id_dtype)
            out.append(c.cuda())
        return out

    def zero_grad(self):
        for m in self.modules.values():
            m.weight.grad = None

    def step(self, cols, dY, id_dtype=torch.int64, pad_rows=False, retain_graph=False):
        out = self.plan.run(self.inputs(cols, id_dtype), pad_rows=pad_rows)
        out.backward(dY.cuda(), retain_graph=retain_graph)
        torch.cuda.synchronize()
        return out

    def grads(self):
        return {k: (m.weight.grad if m.weight.grad is not None else torch.zeros_like(m.weight)) for k, m in self.modules.items()}


class Oracle(object):
    """embed64 over a case; tables of more than COMPACT_ABOVE rows are restated on the rows the batch names (ids, padding
    row and mask ids remapped), every other row's gradient must be zero."""

    def __init__(self, specs, tables, cols, dY, offsets=None):
        self.rows = {}
        small, cols2, specs2 = {}, dict(cols), []
        for key, (w, pad) in tables.items():
            if w.dim() == 2 and w.shape[0] > COMPACT_ABOVE:
                used = [cols[s["name"]].long().reshape(-1) for s in specs if s["table"] == key]
                rows = torch.unique(torch.cat(used))
                self.rows[key] = rows
                hit = (rows == pad).nonzero() if pad is not None else torch.zeros(0)
                small[key] = (w[rows], int(hit) if hit.numel() else None)
            else:
                small[key] = (w, pad)
        for s in specs:
            s = dict(s)
            if s["table"] in self.rows:
                rows = self.rows[s["table"]]
                cols2[s["name"]] = torch.searchsorted(rows, cols[s["name"]].long())
                if s["mask_id"] is not None:
                    hit = (rows == s["mask_id"]).nonzero()
                    s["mask_id"] = int(hit) if hit.numel() else None
            specs2.append(s)
        lookups, self.t64 = lookups64(specs2, small, cols2, offsets=offsets)
        self.out, self.a_out, self.c_out, self.grads = embed64(lookups, dY)

    def check(self, tag, label, out, grads, check_forward=True):
        """Notes max(err / bound) of the forward and of every gradient under ``label`` (the form) and asserts <= 1."""
        ratios = {}
        if check_forward:
            ratios["fwd"] = forward_ratio(out[:, :self.out.shape[1]], self.out, self.a_out, self.c_out)
        for key, t in self.t64.items():
            ent = self.grads.get(id(t))
            got = grads[key].detach()
            if ent is None:
                assert int(torch.count_nonzero(got)) == 0, "%s: %s has a gradient and no lookup" % (tag, key)
                continue
            _, want, A = ent
            if key in self.rows:
                rows = self.rows[key].cuda()
                ratios["bwd " + key] = bound_ratio(got[rows], want, A)
                rest = got.clone()
                rest[rows] = 0
                n_bad = int(torch.count_nonzero(rest))
                assert n_bad == 0, "%s: %s: %d gradient entries outside the looked-up rows" % (tag, key, n_bad)
            else:
                ratios["bwd " + key] = bound_ratio(got, want, A)
        fwd = ratios.get("fwd", 0.0)
        bwd = max([v for k, v in ratios.items() if k != "fwd"] or [0.0])
        print("%s [%s]: forward %.3g, backward %.3g of the bound" % (tag, label, fwd, bwd))
        if check_forward:
            _note("%s forward (err / bound)" % label, fwd, 1.0)
        _note("%s backward (err / bound)" % label, bwd, 1.0)
        worst = max(ratios.items(), key=lambda kv: kv[1])
        assert worst[1] <= 1.0, "%s: %s error is %.3g x the bound (all: %s)" % (
            tag, worst[0], worst[1], ", ".join("%s %.2g" % kv for kv in sorted(ratios.items(), key=lambda kv: -kv[1])))
        return ratios


def _dy(B, width, seed):
    return magnitudes((B, width), torch.Generator().manual_seed(seed))


def _run(specs, tables, cols, dY, tag, label, dtypes=(torch.int64,), pad_rows=False, offsets=None):
    oracle = Oracle(specs, tables, cols, dY, offsets=offsets)
    dev = Device(specs, tables, offsets=offsets, width=dY.shape[1] if offsets is not None else None)
    for dt in dtypes:
        dev.zero_grad()
        out = dev.step(cols, dY, dt, pad_rows=pad_rows)
        oracle.check("%s %s" % (tag, str(dt)[6:]), label, out.detach(), dev.grads())
    return dev, oracle


# ---- the dim grid -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", VEC_NV1 + VEC_NVN + SCALAR_NV1 + SCALAR_NVN)
def test_lookup_grid_of_dims_against_float64(D):
    """One plan per dim (test_embed64_restatement.grid_case): tables of 3, 300, 5000 (no padding row) and 200 000 rows
    (fewer beyond D = 256: 200 000 * 256 / D), a one-id lookup of three of them, SUM / MEAN_ID / MEAN_VALUE histories of
    length 6 sharing the 300-row table, SUM_ID and CONCAT histories, one numeric feature; int64 and float64 id columns;
    6181 samples and 1.  The 3-row table's rows collect ~3 000 lookups each: the long fix-up at every form."""
    big = 200000 if D <= 256 else 200000 * 256 // D
    for B in (6181, 1):
        specs, tables, cols = grid_case(D, B, seed=1000 * D + B, big=big)
        dY = _dy(B, widths(specs, tables)[1], seed=D + B)
        _run(specs, tables, cols, dY, "grid D%d B%d" % (D, B), form(D), dtypes=(torch.int64, torch.float64))


@pytest.mark.parametrize("D", [257, 1028])
def test_dims_without_a_lane_group_form_are_refused_cleanly(D):
    """Scalar D = 257 and vector D = 1028 need more than 256 units per lane group: rbx_embed_fwd, and the backward's
    entry points called directly, return RBX_ERR_UNSUPPORTED (a RuntimeError) before any launch, and the process goes on."""
    from recbox_amd import _lib
    gen = torch.Generator().manual_seed(D)
    tables = {"T": (make_table(50, D, gen), None)}
    specs = [spec("one", table="T")]
    cols = {"one": torch.randint(0, 50, (33,), generator=gen)}
    dev = Device(specs, tables)
    refusal = "too large|not in \\[1,1024\\]"                             # the lane-group dispatch, or the descriptor check at 1028
    with pytest.raises(RuntimeError, match=refusal):
        dev.plan.run(dev.inputs(cols, torch.int64))
    plan = dev.plan.plan
    w = dev.modules["T"].weight
    B, _keep = plan.bind_inputs(dev.inputs(cols, torch.int64))
    plan.bind_params([w], [w])
    assert _lib.lib.rbx_embed_bwd_workspace_size(plan.arr, plan.n, B) == 0
    import re
    assert re.search(refusal, _lib.lib.rbx_last_error().decode())
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    rc = _lib.lib.rbx_embed_sort(plan.arr, plan.n, B, ws.data_ptr(), ws.numel(), None, None)
    assert rc == _lib.RBX_ERR_UNSUPPORTED
    with pytest.raises(RuntimeError):
        _lib.check(rc)
    torch.cuda.synchronize()
    assert int(torch.count_nonzero(ws)) == 0                              # nothing was launched on the workspace
    gen = torch.Generator().manual_seed(1)
    tables = {"T": (make_table(50, 4, gen), None)}                        # ... and the next lookup runs
    _run(specs, tables, cols, _dy(33, 4, 2), "after the refusal of D%d" % D, form(4))


# ---- hot rows -------------------------------------------------------------------------------------------------------
def _hot_case(D, L, seed):
    ids, sign = hot_row_batch(100000, seed=seed, L=L)
    gen = torch.Generator().manual_seed(seed + 1)
    tables = {"T": (make_table(1000, D, gen), None)}
    specs = [spec("hot", table="T", pool="NONE" if L == 1 else "SUM_ID", L=L, mask_id=-1 if L > 1 else None)]
    cols = {"hot": ids.view(-1) if L == 1 else ids}
    return specs, tables, cols, hot_row_dy(sign, D, gen)


@pytest.mark.parametrize("L", [1, 7])
@pytest.mark.parametrize("D", BEYOND)
def test_hot_rows_of_the_generic_lookup_against_float64_and_repeatable(D, L):
    """~100 000 lookups, 70 % of them on one row and 20 % on another (chains of ~4 400 and ~1 250 chunks of 16 sorted pairs
    that segment_fixup_long_kernel splits over workgroups, kw > 1), rows of 250 and 100 lookups, non-zero dY everywhere; as
    a one-id lookup and as SUM_ID histories of 7.  test_embed64_restatement shows that this bar catches ONE lost chunk of
    the hottest row.  Two runs must agree bit for bit."""
    specs, tables, cols, dY = _hot_case(D, L, seed=16)
    dev, oracle = _run(specs, tables, cols, dY, "hot rows D%d L%d" % (D, L), form(D) + " hot rows")
    first = dev.grads()["T"].clone()
    dev.zero_grad()
    dev.step(cols, dY)
    assert torch.equal(dev.grads()["T"], first)


@pytest.mark.parametrize("D", [132, 256])
def test_hot_rows_through_gather_dot_against_float64_and_repeatable(D):
    """The same batch through ops.gather_dot: DotPolicy's instantiation of the three kernels, dW[id] += scale g_r x_r."""
    from recbox_amd import ops
    ids, sign = hot_row_batch(100000, seed=16)
    ids = ids.view(-1)
    gen = torch.Generator().manual_seed(D)
    x = magnitudes((ids.numel(), D), gen)
    w = make_table(1000, D, gen)
    gout = hot_row_dy(sign, 1, gen)
    contrib = 0.5 * gout.double() * x.double()
    want = torch.zeros(1000, D, dtype=torch.float64).index_add_(0, ids, contrib)
    A = torch.zeros(1000, D, dtype=torch.float64).index_add_(0, ids, contrib.abs())

    def run():
        wc = w.cuda().requires_grad_(True)
        out = ops.gather_dot(x.cuda(), [ids.cuda()], wc, scale=0.5)
        out.backward(gout.cuda())
        torch.cuda.synchronize()
        return wc.grad.clone()

    a, b = run(), run()
    r = bound_ratio(a, want, A)
    _note("%s hot rows gather_dot backward (err / bound)" % form(D), r, 1.0)
    assert r <= 1.0, "gather_dot D%d: %.3g x the bound" % (D, r)
    assert torch.equal(a, b)


@pytest.mark.parametrize("D", [16, 132])
def test_zero_upstream_gradient_on_the_hot_rows_samples(D):
    """dY exactly zero on every sample that names the hottest row: its chunks' tails are flagged zero and the fix-up walks
    flags (kFlagZero); the row's gradient must be exactly zero (A = 0), every other row within the bound."""
    specs, tables, cols, dY = _hot_case(D, 1, seed=16)
    dY[cols["hot"] == 7] = 0
    _run(specs, tables, cols, dY, "zero dY on the hot row D%d" % D, form(D) + " hot rows")


# ---- long histories -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [65, 200, 300])
@pytest.mark.parametrize("D", [4, 64, 128, 256])
def test_long_histories_with_masked_ids_against_float64(D, L):
    """MEAN_ID and SUM over one 300-row table, ~30 % of the ids masked beyond the ragged tails, ~10 % of the samples fully
    masked (count 0: eps = 1e-8 makes that 0 * 1e8 = 0), and MEAN_ID with eps = 0 over histories that keep at least one id
    (0 / 0 is the reference's answer otherwise): every SG of embed_seq_kernel, several compaction chunks per sample."""
    gen = torch.Generator().manual_seed(D * 1000 + L)
    B = 61
    tables = {"T": (make_table(300, D, gen, pad=0), 0)}
    specs = [spec("mean", table="T", pool="MEAN_ID", L=L, mask_id=0, eps=1e-8),
             spec("sum", table="T", pool="SUM", L=L),
             spec("mean0", table="T", pool="MEAN_ID", L=L, mask_id=0, eps=0.0)]
    cols = {"mean": history(300, B, L, gen, masked_frac=0.3, empty_frac=0.1),
            "sum": history(300, B, L, gen, masked_frac=0.3, empty_frac=0.1),
            "mean0": history(300, B, L, gen, masked_frac=0.3)}
    cols["mean0"][:, 0] = torch.randint(1, 300, (B,), generator=gen)
    assert bool((cols["mean"] == 0).all(1).any())
    _run(specs, tables, cols, _dy(B, 3 * D, L), "histories D%d L%d" % (D, L), form(D) + " histories",
         dtypes=(torch.int64, torch.float64))


# ---- scalar fallback, mixed dims -------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad_rows", [False, True])
def test_vector_dim_behind_an_unaligned_field_runs_the_scalar_form(pad_rows):
    """A D = 256 field behind a D = 7 field: its offset is not a multiple of 4, so its forward launch and the whole
    backward call are scalar (<64, 4, false>: the widest scalar form), with and without 16-byte padded output rows."""
    gen = torch.Generator().manual_seed(7256)
    B = 3001
    tables = {"T7": (make_table(50, 7, gen, pad=0), 0), "T256": (make_table(300, 256, gen, pad=0), 0),
              "T3": (make_table(3, 256, gen), None)}
    specs = [spec("a", table="T7"), spec("b", table="T256"), spec("c", table="T256", pool="SUM", L=6), spec("d", table="T3")]
    cols = {"a": torch.randint(0, 50, (B,), generator=gen), "b": torch.randint(0, 300, (B,), generator=gen),
            "c": history(300, B, 6, gen), "d": torch.randint(0, 3, (B,), generator=gen)}
    _run(specs, tables, cols, _dy(B, widths(specs, tables)[1], 3), "D7 + D256 pad_rows=%s" % pad_rows,
         form(256, vec=False) + " fallback", pad_rows=pad_rows)


def test_narrow_and_wide_fields_in_one_plan():
    """D = 4 and D = 256 in one plan: the lane group follows the widest row (G = 64), the narrow row uses one lane of it."""
    gen = torch.Generator().manual_seed(4256)
    B = 3001
    tables = {"T4": (make_table(3, 4, gen), None), "T256": (make_table(300, 256, gen, pad=0), 0),
              "U4": (make_table(5000, 4, gen, pad=0), 0)}
    specs = [spec("a", table="T4"), spec("b", table="T256"), spec("c", table="U4", pool="MEAN_ID", L=6, mask_id=0, eps=1e-16),
             spec("d", table="T256", pool="SUM_ID", L=6, mask_id=0)]
    cols = {"a": torch.randint(0, 3, (B,), generator=gen), "b": torch.randint(0, 300, (B,), generator=gen),
            "c": history(5000, B, 6, gen), "d": history(300, B, 6, gen)}
    _run(specs, tables, cols, _dy(B, widths(specs, tables)[1], 5), "D4 + D256", form(256) + " mixed dims")


# ---- accumulation, persistent gradients -------------------------------------------------------------------------------
@pytest.mark.parametrize("D", BEYOND)
def test_one_table_in_two_plans_and_backward_twice_over_one_sort(D):
    """Two Plans that read one table in one backward pass: the second node adopts the gradient the first one published and
    adds its rows into it (accumulate = 1: the reduce prefetches the old row); against the restatement of both lookups.
    Then a second backward over the same forwards and sorts: exactly twice the gradient."""
    gen = torch.Generator().manual_seed(D + 77)
    B = 3001
    tables = {"T": (make_table(300, D, gen, pad=0), 0), "T3": (make_table(3, D, gen), None)}
    specs = [spec("a", table="T"), spec("h", table="T3"), spec("b", table="T", pool="SUM", L=6), spec("g", table="T3")]
    cols = {"a": torch.randint(0, 300, (B,), generator=gen), "h": torch.randint(0, 3, (B,), generator=gen),
            "b": history(300, B, 6, gen), "g": torch.randint(0, 3, (B,), generator=gen)}
    dY = _dy(B, 4 * D, D)
    oracle = Oracle(specs, tables, cols, dY)
    first = Device(specs[:2], tables)
    second = Device(specs[2:], tables, modules=first.modules)               # the SAME module objects: one parameter each
    out1 = first.plan.run(first.inputs(cols, torch.int64))
    out2 = second.plan.run(second.inputs(cols, torch.int64))
    dYc = dY.cuda()
    torch.autograd.backward([out1, out2], [dYc[:, :2 * D].contiguous(), dYc[:, 2 * D:].contiguous()], retain_graph=True)
    torch.cuda.synchronize()
    oracle.check("two plans D%d" % D, form(D) + " accumulate", torch.cat([out1, out2], 1).detach(), first.grads())
    once = {k: g.clone() for k, g in first.grads().items()}
    torch.autograd.backward([out1, out2], [dYc[:, :2 * D].contiguous(), dYc[:, 2 * D:].contiguous()])
    torch.cuda.synchronize()
    for k, g in first.grads().items():
        assert torch.equal(g, 2 * once[k]), "second backward over the same sort differs: " + k


@pytest.mark.parametrize("D", BEYOND)
def test_persistent_gradients_keep_no_residue_of_the_previous_step(D):
    """ops.config.reuse_grad_buffers = "all": the gradients live in one persistent buffer and rezero_rows_kernel clears the
    rows the previous step's sorted ids name (lanes = 64 per row from D = 256 on: rows wider than the lane group).  Two steps
    over different batches; the second step's gradient meets the bound, rows it did not look up are exactly zero."""
    from recbox_amd import ops
    gen = torch.Generator().manual_seed(D + 99)
    B = 2000
    tables = {"T": (make_table(5000, D, gen, pad=0), 0), "S": (make_table(300, D, gen), None)}
    specs = [spec("a", table="T"), spec("b", table="S", pool="SUM", L=6), spec("c", table="T", pool="MEAN_ID", L=6, mask_id=0,
                                                                             eps=1e-16)]
    dev = Device(specs, tables)
    old = ops.config.reuse_grad_buffers
    try:
        ops.config.reuse_grad_buffers = "all"
        for step, Bk in enumerate((B, B - 300)):
            cols = {"a": torch.randint(0, 5000, (Bk,), generator=gen), "b": history(300, Bk, 6, gen),
                    "c": history(5000, Bk, 6, gen)}
            dY = _dy(Bk, 3 * D, D + step)
            dev.zero_grad()
            out = dev.step(cols, dY)
            Oracle(specs, tables, cols, dY).check("persistent D%d step %d" % (D, step), form(D) + " persistent",
                                                  out.detach(), dev.grads())
    finally:
        ops.config.reuse_grad_buffers = old


@pytest.mark.parametrize("D", [16, 132])
def test_every_id_of_the_batch_masked(D):
    """SUM_ID and MEAN_ID histories whose ids are all the mask id: no sorted pair carries a row; outputs and gradients are
    exactly zero."""
    gen = torch.Generator().manual_seed(D)
    B = 257
    tables = {"T": (make_table(300, D, gen), None)}
    specs = [spec("s", table="T", pool="SUM_ID", L=6, mask_id=0), spec("m", table="T", pool="MEAN_ID", L=6, mask_id=0, eps=1e-8)]
    cols = {"s": torch.zeros(B, 6, dtype=torch.long), "m": torch.zeros(B, 6, dtype=torch.long)}
    dev, _ = _run(specs, tables, cols, _dy(B, 2 * D, 1), "all masked D%d" % D, form(D) + " all masked")
    assert int(torch.count_nonzero(dev.grads()["T"])) == 0
