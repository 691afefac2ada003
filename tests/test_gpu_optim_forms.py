"""The sparse-row optimiser step on the C ABI -- rbx_embed_sparse_update, rbx_fm_sparse_update, rbx_embed_csr_sparse_update,
rbx_opt_advance -- and recbox_amd.optim over them, against the float64 restatement of oracle/optim64.py at every form
rbx_optim.hip dispatches: |got - want| <= 64 eps32 A + tiny element by element on the looked-up rows; every other row of
the table, of both state tensors and of the gradient BIT-IDENTICAL.  Each case is sort -> backward -> update; the oracle
steps the device's own gradient buffer on the rows computed here from the ids.

Forms (rbx_optim.hip)
  launch_pairs       kUpdFields = 32 plan slots per launch; per pack: vec iff every table of it has dim % 4 == 0 and a
                     16-byte aligned table, gradient and state (upd_vec_ok), G = lanes_for(largest dim of the pack, vec) =
                     next power of two >= dim / 4 (vec) or dim (scalar), at most 64; blocks = ceil(lookups / (256 / G)),
                     capped at kCUs * 64 = 16 384 -> at G = 64 (4 pairs per block) the grid-stride loop runs a second trip
                     from 65 537 lookups.
       dim     1        10        16        67            128       260                (16, 10, 16)    (4, 128)
       form    s G=1    s G=16    v G=4     s G=64 x2     v G=32    v G=64 x2 trips    s G=16          v G=32, dim 4 on lane 0
  ta_sparse_update   kTaUpdTables = 32 tier-A tables per launch; a lane group per table row, stepped iff the row's bit is set
                     in the bitmap of ANY of the NB = ceil(B / 2048) sample blocks of ANY field that reads the table.
  fm_plan's tier rule: emb != NULL, D <= 64, vocab <= 4096 (and 2^20 floats of gradient in all): tier A (bitmaps); else
                     tier B (sorted pairs).  emb == NULL is one tier (B) with D = 1, G = 1.

Findings
  rbx_fm_sparse_update refused a packed LR table (or a missing state tensor) of a TIER-A table only after tier B had been
  stepped: "nothing is written" did not hold.  Fixed (every refusal now comes before the first launch) and pinned by
  test_fm_refusals_write_nothing.
  The by-value step size of SparseAdam came from double betas (verdict (a) of oracle/optim64.py): fixed in optim.py,
  pinned by test_opt_advance_counts_exactly_and_writes_the_step_size_of_its_step (by-value against the device's).

Worst err / bound observed on the MI355X (145 cases, 11 s for the file, the slowest case 1.1 s; the ledger of
conftest._note has every label)
  rbx_embed_sparse_update 0.015    rbx_fm_sparse_update 0.015    rbx_embed_csr_sparse_update 0.015
  recbox_amd.optim: embed 0.017, fm_fused 0.014, bags 0.016, dense fallback 0.012 (0.57 while it took 1 - beta from the
  double betas)      rbx_opt_advance: 0.20 of K eps32; by-value against the device's 0.20 as well

Mutation check (scratch builds of rbx_optim.hip, not committed): failed cases of this file / tests/test_gpu_optim.py /
tests/test_gpu_embed_csr_optim.py
  the parent's rbx_optim.hip                          1 (test_fm_refusals_write_nothing[tier A])  / 0 / 0
  1  no run-head test keys[i - 1] == key              34 / 13 / 31
  2  slot without - slot_lo                           all 9 cases of test_embed_more_than_32_plan_slots / 0 / 0 -- the pairs
     of slots 0 .. 31 then index the second pack's unfilled entries: the first such case ended in an illegal memory
     access, and what the file reported after it in that process does not count
  3  weight decay ignored under Adam                  37 / 0 / 0
  4  only block 0 of the tier-A bitmap                6 (test_fm_second_tier_a_block) / 0 / 0
"""
import ctypes
import math

import pytest
import torch

from conftest import _note
from oracle import optim64 as O
from test_optim64_restatement import table_and_state

pytestmark = pytest.mark.gpu

EPS32, TINY, C = O.EPS32, O.TINY, O.C_BOUND
RULES = ["sgd", "adagrad", "adam"]
KIND = {"sgd": O.SGD, "adagrad": O.ADAGRAD, "adam": O.ADAM}
WDS = [0.0, 0.05]
FROZEN_STATE = 123.0
NO_ID = -(1 << 63)
K_UPD_FIELDS, K_TA_TABLES, K_TA_BLOCK, K_CUS = 32, 32, 2048, 256


def hp_of(rule):
    """Hyper-parameters of step 3 (so that no step size is a round number); lr is the folded, by-value step size."""
    if rule == "sgd":
        return dict(lr=0.05)
    if rule == "adagrad":
        return dict(lr=O.step_size(O.ADAGRAD, 0.05, lr_decay=0.1, t=3)[0], eps=1e-10)
    return dict(lr=O.step_size(O.ADAM, 0.01, 0.9, 0.999, t=3)[0], beta1=0.9, beta2=0.999, eps=1e-8)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _opt(rule, hp, wd, d_step=None):
    from recbox_amd import _lib
    return _lib.rbx_opt_t(KIND[rule], hp["lr"], hp.get("beta1", 0.0), hp.get("beta2", 0.0), hp.get("eps", 0.0), wd,
                          d_step.data_ptr() if d_step is not None else None)


def check(what, got, want, A):
    got = got.detach().double().cpu()
    bound = C * EPS32 * A + TINY
    ratio = float(((got - want).abs() / bound).max()) if got.numel() else 0.0
    assert bool(torch.isfinite(got).all()), "%s: non-finite" % what
    _note(what, ratio, 1.0)
    assert ratio <= 1.0, "%s: err / bound = %.3f" % (what, ratio)
    return ratio


class Param(object):
    """One table with its gradient and state on the device.  ``store``: the [V, stride] storage the table lives in
    (stride == D unless packed); ``w`` is the [V, D] view of it the optimiser steps."""

    def __init__(self, V, D, gen, stride=None, offset_state=False, frozen=False):
        self.V, self.D, self.frozen = V, D, frozen
        w, s1, s2 = table_and_state((V, D), gen)
        self.stride = stride or D
        self.store = torch.randn(V, self.stride, generator=gen).mul_(0.1).cuda()
        self.store[:, :D] = w.cuda()
        self.g = None if frozen else torch.zeros(V, D, device="cuda")
        if offset_state:          # 4 bytes past a 16-byte boundary: upd_vec_ok refuses the float4 form
            self._raw = [torch.zeros(V * D + 4, device="cuda") for _ in range(2)]
            self.s1, self.s2 = [r[1:1 + V * D].view(V, D) for r in self._raw]
            self.s1.copy_(s1)
            self.s2.copy_(s2)
            assert self.s1.data_ptr() % 16 == 4
        else:
            self.s1, self.s2 = s1.cuda(), s2.cuda()
        if frozen:
            self.s1.fill_(FROZEN_STATE)
            self.s2.fill_(FROZEN_STATE)
        self.rows, self.never = None, []

    @property
    def w(self):
        return self.store[:, :self.D]

    def snap(self):
        return dict(store=self.store.clone(), s1=self.s1.clone(), s2=self.s2.clone(), g=None if self.g is None else self.g.clone())

    def restore(self, snap):
        self.store.copy_(snap["store"])
        self.s1.copy_(snap["s1"])
        self.s2.copy_(snap["s2"])
        if self.g is not None:
            self.g.copy_(snap["g"])


def verify(tag, rule, hp, wd, p, before, want_moved=True):
    """``p`` (after one step) against the oracle's step from ``before`` on ``p.rows``; returns the worst err / bound."""
    D = p.D
    after = p.snap()
    if p.g is not None:
        assert torch.equal(after["g"], before["g"]), "%s: the gradient was written" % tag
    assert torch.equal(after["store"][:, D:], before["store"][:, D:]), "%s: the columns beside a packed table were written" % tag
    if p.frozen or p.rows is None:
        for k in ("store", "s1", "s2"):
            assert torch.equal(after[k], before[k]), "%s: a frozen slot's %s was written" % (tag, k)
        return 0.0
    rows = p.rows
    assert rows.numel() > 0
    (w, a_w), (n1, a1), (n2, a2) = O.step_rows(KIND[rule], before["store"][:, :D], before["g"], rows, before["s1"], before["s2"],
                                               weight_decay=wd, **hp)
    worst = check("%s w" % tag, after["store"][:, :D], w, a_w)
    mask = torch.zeros(p.V, dtype=torch.bool)
    mask[rows] = True
    off = (~mask).cuda()
    for k in ("store", "s1", "s2"):
        assert torch.equal(after[k][off], before[k][off]), "%s: a row nobody looked up changed in %s" % (tag, k)
    for r in p.never:
        if 0 <= r < p.V:
            assert not bool(mask[r]), (tag, r)
            for k in ("store", "s1", "s2"):
                assert torch.equal(after[k][r], before[k][r]), "%s: row %d (padding / masked / outside) changed in %s" % (tag, r, k)
    if want_moved and (rule != "sgd" or wd or bool((before["g"][rows.cuda()] != 0).any())):
        assert not torch.equal(after["store"][mask.cuda()], before["store"][mask.cuda()])
    if rule == "sgd":
        assert torch.equal(after["s1"], before["s1"]) and torch.equal(after["s2"], before["s2"]), "%s: SGD wrote state" % tag
        return worst
    worst = max(worst, check("%s state1" % tag, after["s1"], n1, a1))
    if rule == "adam":
        worst = max(worst, check("%s state2" % tag, after["s2"], n2, a2))
    else:
        assert torch.equal(after["s2"], before["s2"]), "%s: Adagrad wrote the second state" % tag
    return worst


def zero_grad_rows_move(tag, rule, p, before):
    """Looked-up rows whose summed gradient is exactly zero exist; under Adam (no weight decay) they moved by the decayed
    first moment -- the oracle says by how much, this says that they were not skipped."""
    rows = p.rows.cuda()
    zero = rows[(before["g"][rows] == 0).all(dim=1)]
    assert zero.numel() > 0, "%s: no looked-up row with a zero gradient" % tag
    if rule == "adam":
        assert bool((p.w[zero] != before["store"][zero][:, :p.D]).any(dim=1).all()), "%s: a zero-gradient row was not stepped" % tag
        assert bool((p.s1[zero] != before["s1"][zero]).any(dim=1).all()) and bool((p.s2[zero] != before["s2"][zero]).any(dim=1).all())


def set_field(f, ids, p, L=1, pad=None, mask=None, pool=0, out_off=0, dim=None, table=None, grad="own", stride=0):
    f.ids = ids.data_ptr()
    f.ids_stride_b = ids.stride(0)
    f.ids_stride_l = ids.stride(1) if ids.dim() == 2 else 0
    f.ids_dtype = {torch.int32: 0, torch.int64: 1}[ids.dtype]
    f.table = table if table is not None else p.store.data_ptr()
    g = p.g if grad == "own" else grad
    f.grad = g.data_ptr() if g is not None else None
    f.vocab, f.dim, f.seq_len, f.kind, f.pool, f.eps = p.V, (dim or p.D), L, 0, pool, 0.0
    f.padding_idx = NO_ID if pad is None else pad
    f.mask_id = NO_ID if mask is None else mask
    f.out_off, f.table_stride = out_off, stride


def _ids(V, shape, gen, zero_tail, reserve=16, lo=0):
    """ids in [lo, V - reserve) for the samples in front, in [V - reserve, V) for the last ``zero_tail`` samples (whose
    upstream gradient is exactly zero): the rows of that band are looked up and have a zero summed gradient."""
    B = shape[0]
    reserve = min(reserve, max(V // 4, 1)) if zero_tail else 0
    ids = torch.randint(lo, max(V - reserve, lo + 1), shape, generator=gen)
    if zero_tail and reserve:
        ids[B - zero_tail:] = torch.randint(V - reserve, V, ids[B - zero_tail:].shape, generator=gen)
    return ids


def _looked_up(ids, V, pad=None, mask=None):
    live = ids.reshape(-1).long()
    live = live[(live >= 0) & (live < V)]
    if pad is not None:
        live = live[live != pad]
    if mask is not None:
        live = live[live != mask]
    return torch.unique(live)


# ======== rbx_embed_sparse_update =============================================================================================
class Embed(object):
    """feats: (table key, V, D, options) per feature; options: L, pad, mask (with L > 1: POOL_SUM_ID), i32, frozen, oob,
    offset_state.  Features with one key share table, gradient and state."""

    def __init__(self, feats, B=65, seed=0, zero_tail=8):
        from recbox_amd import _lib
        from recbox_amd._lib import check as ok, lib
        gen = torch.Generator().manual_seed(4000 + seed)
        self.B, self.n = B, len(feats)
        self.params, self.order, self.of_feat = {}, [], []
        self.arr = (_lib.rbx_field_t * self.n)()
        self.keep, off = [], 0
        rows = {}
        for i, (key, V, D, o) in enumerate(feats):
            if key not in self.params:
                self.params[key] = Param(V, D, gen, offset_state=o.get("offset_state", False), frozen=o.get("frozen", False))
                self.order.append(key)
                rows[key] = []
            p = self.params[key]
            L, pad, mask = o.get("L", 1), o.get("pad"), o.get("mask")
            lo = 2 if (pad is not None or mask is not None) else 0
            ids = _ids(V, (B, L) if L > 1 else (B,), gen, zero_tail, lo=lo)
            flat = ids.view(-1)
            if pad is not None:
                flat[0] = pad
                p.never.append(pad)
            if mask is not None:
                flat[1] = mask
                p.never.append(mask)
            if o.get("oob"):
                flat[2] = V + 13                            # outside [0, vocab): flagged, never looked up
            ids = ids.to(torch.int32 if o.get("i32") else torch.int64).cuda()
            self.keep.append(ids)
            set_field(self.arr[i], ids, p, L=L, pad=pad, mask=mask, pool=(_lib.POOL_SUM_ID if L > 1 else _lib.POOL_NONE), out_off=off)
            off += D
            self.of_feat.append(p)
            if not p.frozen:
                rows[key].append(_looked_up(ids.cpu(), V, pad, mask))
        for key, p in self.params.items():
            p.rows = torch.unique(torch.cat(rows[key])) if rows[key] else None
        self.width = off
        # the upstream gradient of a batch-mean loss; exactly zero for the last ``zero_tail`` samples
        self.dY = torch.randn(B, off, generator=gen).div_(B).cuda()
        if zero_tail:
            self.dY[B - zero_tail:] = 0.0
        self.ws_bytes = lib.rbx_embed_bwd_workspace_size(self.arr, self.n, B)
        assert self.ws_bytes > 0
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device="cuda")
        self.status = torch.zeros(1, dtype=torch.int32, device="cuda")
        ok(lib.rbx_embed_sort(self.arr, self.n, B, _ptr(self.ws), self.ws_bytes, _ptr(self.status), _stream()))
        ok(lib.rbx_embed_bwd(self.arr, self.n, B, _ptr(self.dY), self.width, None, 0, _ptr(self.ws), self.ws_bytes, _stream()))
        torch.cuda.synchronize()
        self.flagged = bool(int(self.status.item()) & 1)
        self.start = dict((k, p.snap()) for k, p in self.params.items())

    def reset(self):
        for k, p in self.params.items():
            p.restore(self.start[k])

    def update(self, rule, hp, wd, d_step=None, expect=0):
        from recbox_amd._lib import lib
        n_state = {"sgd": 0, "adagrad": 1, "adam": 2}[rule]
        arrs = []
        for k in range(2):
            a = (ctypes.c_void_p * self.n)()
            for i, p in enumerate(self.of_feat):
                a[i] = (p.s1, p.s2)[k].data_ptr()
            arrs.append(a if k < n_state else None)
        opt = _opt(rule, hp, wd, d_step)
        rc = lib.rbx_embed_sparse_update(self.arr, self.n, self.B, _ptr(self.ws), self.ws_bytes, ctypes.byref(opt), arrs[0], arrs[1],
                                         _stream())
        torch.cuda.synchronize()
        assert rc == expect, rc
        return rc

    def run(self, tag, rule, zero_rows_of=None):
        worst = 0.0
        hp = hp_of(rule)
        for wd in WDS:
            self.reset()
            self.update(rule, hp, wd)
            for k in self.order:
                p = self.params[k]
                worst = max(worst, verify("%s %s wd=%g %s" % (tag, rule, wd, k), rule, hp, wd, p, self.start[k]))
                if zero_rows_of == k and wd == 0.0:
                    zero_grad_rows_move(tag, rule, p, self.start[k])
        return worst


# V = 211 > 3 B: most rows are not looked up.  dim -> form: see the module docstring.
@pytest.mark.parametrize("dim", [1, 10, 16, 67, 128, 260])
@pytest.mark.parametrize("rule", RULES)
def test_embed_every_dim_form(rule, dim):
    """Three tables of one dim (int64 ids; int32 ids with padding_idx; a table of 7 rows that the batch covers whole), the
    last 8 samples with a zero upstream gradient: looked-up rows with a zero summed gradient are stepped."""
    c = Embed([("a", 211, dim, {}), ("b", 307, dim, {"i32": True, "pad": 0}), ("c", 7, dim, {})], seed=dim)
    c.run("embed dim %d" % dim, rule, zero_rows_of="a")


MIXED = {
    # one table of dim 10 sends the whole pack to the scalar form, G = lanes_for(16, false) = 16
    "16x10x16 scalar pack": [("a", 211, 16, {}), ("b", 211, 10, {}), ("c", 211, 16, {"i32": True})],
    # float4 pack, G = lanes_for(128, true) = 32: the dim-4 table is one float4 on lane 0, lanes 1 .. 31 idle
    "4x128 idle lanes": [("a", 211, 4, {}), ("b", 211, 128, {})],
    # a frozen feature (no gradient: no plan slot) in front: plan slot c is feature c + 1, state arrays are by FEATURE
    "frozen in front": [("f", 50, 16, {"frozen": True}), ("a", 211, 16, {}), ("b", 211, 16, {"i32": True})],
    # a sequence feature (L = 5, POOL_SUM_ID) with padding_idx 0 and mask id 1, and one id outside [0, vocab)
    "sequence pad mask oob": [("a", 211, 16, {"L": 5, "pad": 0, "mask": 1, "oob": True}), ("b", 211, 16, {})],
    "sequence pad mask oob i32 scalar": [("a", 211, 10, {"L": 5, "pad": 0, "mask": 1, "oob": True, "i32": True}), ("b", 211, 10, {})],
}


@pytest.mark.parametrize("name", list(MIXED))
@pytest.mark.parametrize("rule", RULES)
def test_embed_mixed_frozen_sequence(rule, name):
    c = Embed(MIXED[name], seed=len(name))
    if "oob" in name:
        assert c.flagged, "the out-of-range id was not flagged"
        assert not bool((c.params["a"].rows == 211 + 13).any())
    c.run("embed %s" % name, rule, zero_rows_of="a" if "frozen" not in name else "b")
    if "sequence" in name:
        assert c.params["a"].never == [0, 1]


@pytest.mark.parametrize("dim", [16, 10])
@pytest.mark.parametrize("rule", ["adagrad", "adam"])
def test_embed_two_features_on_one_table_step_a_row_once(rule, dim):
    """Two features over ONE table of 40 rows at B = 65: nearly every row is named by both, and by many samples.  A row
    stepped twice is invisible to SGD with a summed gradient; Adagrad would add g^2 twice, Adam decay twice."""
    c = Embed([("t", 40, dim, {}), ("u", 211, dim, {}), ("t", 40, dim, {"i32": True})], seed=3, zero_tail=0)
    ids0, ids2 = c.keep[0].cpu().long(), c.keep[2].cpu().long()
    assert int(torch.isin(torch.unique(ids0), torch.unique(ids2)).sum()) > 10
    c.run("embed shared table dim %d" % dim, rule)


@pytest.mark.parametrize("rule", RULES)
def test_embed_misaligned_state_takes_the_scalar_form_bit_for_bit(rule):
    """dim 16 with a state tensor 4 bytes off a 16-byte boundary: upd_vec_ok -> the scalar form of the whole pack.  Same
    ids, tables and gradients as the aligned run (same seed): bit-equal tables and state, and within the oracle's bound."""
    feats = [("a", 211, 16, {}), ("b", 211, 16, {"i32": True, "pad": 0})]
    al = Embed(feats, seed=11)
    mis = Embed([(k, V, D, dict(o, offset_state=(k == "b"))) for k, V, D, o in feats], seed=11)
    hp = hp_of(rule)
    for wd in WDS:
        al.reset(), mis.reset()
        al.update(rule, hp, wd), mis.update(rule, hp, wd)
        for k in al.order:
            a, m = al.params[k], mis.params[k]
            assert torch.equal(al.start[k]["g"], mis.start[k]["g"])
            assert torch.equal(a.store, m.store) and torch.equal(a.s1, m.s1) and torch.equal(a.s2, m.s2), (rule, wd, k)
            verify("embed misaligned state %s wd=%g %s" % (rule, wd, k), rule, hp, wd, m, mis.start[k])


def _many(n):
    """n features at B = 65: slots 0 .. 31 are dim 8 (first pack: float4, G = 2); from slot 33 on dim 5 (second pack: scalar,
    G = lanes_for(8, false) = 8); slot 32 reads the table of slot 31, so that table's pairs straddle the pack boundary --
    a run of equal keys is stepped by the pack that holds the slot of its HEAD pair, and by no other."""
    feats = []
    for i in range(n):
        if i < K_UPD_FIELDS:
            feats.append(("t%d" % i, 9 + i % 5, 8, {"i32": bool(i % 2)}))
        elif i == K_UPD_FIELDS:
            feats.append(("t%d" % (K_UPD_FIELDS - 1), 9 + (K_UPD_FIELDS - 1) % 5, 8, {}))
        else:
            feats.append(("t%d" % i, 9 + i % 5, 5, {"i32": bool(i % 2)}))
    return feats


@pytest.mark.parametrize("n", [33, 34, 64])
@pytest.mark.parametrize("rule", RULES)
def test_embed_more_than_32_plan_slots(rule, n):
    """33: the second pack is slot 32 alone (float4, the shared table); 34 and 64 (RBX_MAX_FIELDS): it is scalar."""
    c = Embed(_many(n), seed=n, zero_tail=0)
    assert len(c.order) == n - 1
    c.run("embed %d slots" % n, rule)


@pytest.mark.parametrize("rule", RULES)
def test_embed_past_the_grid_cap(rule):
    """dim 256 (float4, G = 64: 4 pairs per block), a sequence feature of L = 64 at B = 1026: 65 664 lookups > kCUs * 64 * 4 =
    65 536 -> 16 384 blocks and a second trip of the grid-stride loop, over 300 rows."""
    B, L = 1026, 64
    assert B * L > K_CUS * 64 * 4 and (B - 1) * L <= K_CUS * 64 * 4 + L
    c = Embed([("a", 300, 256, {"L": L, "pad": 0, "mask": 1})], B=B, seed=5)
    c.run("embed grid cap", rule, zero_rows_of="a")


# ======== rbx_fm_sparse_update ================================================================================================
class Fm(object):
    """fields: (key, V, options); options: pad, frozen_emb, stride (packed embedding storage), force (ids put in front).
    Fields with one key share the embedding table and the LR table.  mode: "both", "emb" (lr == NULL), "lr" (emb == NULL)."""

    def __init__(self, fields, D, B=65, mode="both", seed=0, zero_tail=8, tail_only=None):
        from recbox_amd import _lib
        from recbox_amd._lib import check as ok, lib
        gen = torch.Generator().manual_seed(7000 + seed)
        self.B, self.n, self.D, self.mode = B, len(fields), D, mode
        self.emb, self.lr, self.order, self.keep = {}, {}, [], []
        self.ea = (_lib.rbx_field_t * self.n)() if mode != "lr" else None
        self.la = (_lib.rbx_field_t * self.n)() if mode != "emb" else None
        self.e_of, self.l_of = [], []
        rows = {}
        for i, (key, V, o) in enumerate(fields):
            if key not in rows:
                rows[key] = []
                self.order.append(key)
                if mode != "lr":
                    self.emb[key] = Param(V, D, gen, stride=o.get("stride"), frozen=o.get("frozen_emb", False))
                if mode != "emb":
                    self.lr[key] = Param(V, 1, gen)
            pad = o.get("pad")
            ids = _ids(V, (B,), gen, zero_tail, lo=1 if pad == 0 else 0)
            for j, r in enumerate(o.get("force", [])):
                ids[j] = r
            if tail_only is not None and key == tail_only[0]:
                ids[ids == tail_only[1]] = tail_only[1] - 1
                ids[B - 2] = tail_only[1]                    # a row that only a sample of the LAST block names
            ids = ids.to(torch.int32 if i % 2 else torch.int64).cuda()
            self.keep.append(ids)
            if self.ea is not None:
                p = self.emb[key]
                set_field(self.ea[i], ids, p, pad=pad, stride=(p.stride if p.stride != D else 0))
            if self.la is not None:
                set_field(self.la[i], ids, self.lr[key], pad=pad)
            self.e_of.append(self.emb.get(key))
            self.l_of.append(self.lr.get(key))
            rows[key].append(_looked_up(ids.cpu(), V, pad))
            for q in (self.emb.get(key), self.lr.get(key)):
                if q is not None and pad is not None and pad not in q.never:
                    q.never.append(pad)
        for key in self.order:
            for q in (self.emb.get(key), self.lr.get(key)):
                if q is not None:
                    q.rows = torch.unique(torch.cat(rows[key]))
        self.g = torch.randn(B, generator=gen).div_(B).cuda()                # dL/dlogit of a batch-mean loss
        if zero_tail:
            self.g[B - zero_tail:] = 0.0
        self.ssum = torch.randn(B, D, generator=gen).mul_(0.3).cuda()
        self.gb = torch.zeros(1, device="cuda")
        self.ws_bytes = lib.rbx_fm_bwd_workspace_size(self.ea, self.la, self.n, B)
        assert self.ws_bytes > 0
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device="cuda")
        ok(lib.rbx_fm_sort(self.ea, self.la, self.n, B, _ptr(self.ws), self.ws_bytes, None, _stream()))
        ok(lib.rbx_fm_bwd(self.ea, self.la, self.n, B, _ptr(self.g), _ptr(self.ssum), _ptr(self.gb), 0, 3, _ptr(self.ws), self.ws_bytes,
                          _stream()))
        torch.cuda.synchronize()
        self.all = [("emb " + k, p) for k, p in self.emb.items()] + [("lr " + k, p) for k, p in self.lr.items()]
        self.start = dict((n, p.snap()) for n, p in self.all)

    def reset(self):
        for n, p in self.all:
            p.restore(self.start[n])

    def update(self, rule, hp, wd, d_step=None):
        from recbox_amd._lib import lib
        n_state = {"sgd": 0, "adagrad": 1, "adam": 2}[rule]

        def arrays(of):
            out = []
            for k in range(2):
                a = (ctypes.c_void_p * self.n)()
                for i, p in enumerate(of):
                    a[i] = (p.s1, p.s2)[k].data_ptr() if p is not None else None
                out.append(a if (k < n_state and any(p is not None for p in of)) else None)
            return out
        e, l = arrays(self.e_of), arrays(self.l_of)
        opt = _opt(rule, hp, wd, d_step)
        rc = lib.rbx_fm_sparse_update(self.ea, self.la, self.n, self.B, _ptr(self.ws), self.ws_bytes, ctypes.byref(opt), e[0], e[1],
                                      l[0], l[1], _stream())
        torch.cuda.synchronize()
        return rc

    def run(self, tag, rule, zero_rows_of=None, wds=WDS):
        worst, hp = 0.0, hp_of(rule)
        for wd in wds:
            self.reset()
            assert self.update(rule, hp, wd) == 0
            for n, p in self.all:
                worst = max(worst, verify("%s %s wd=%g %s" % (tag, rule, wd, n), rule, hp, wd, p, self.start[n]))
                if zero_rows_of is not None and n.endswith(" " + zero_rows_of) and wd == 0.0 and not p.frozen:
                    zero_grad_rows_move(tag + " " + n, rule, p, self.start[n])
        return worst


def _fm_fields():
    """Both tiers in one call (fm_plan: vocab <= 4096 -> tier A): "a" 37 rows with padding row 0 named by the batch; "s" 70
    rows (not a multiple of 32) read by TWO fields, ids 31, 32 and V - 1 = 69 forced (bits 31 of word 0, 0 of word 1, the
    last bit of the last word); "b" 5000 and "c" 4500 rows: tier B, "c" read by two fields."""
    return [("a", 37, {"pad": 0, "force": [0, 5]}), ("s", 70, {"force": [31, 32, 69]}), ("b", 5000, {"pad": 0, "force": [0]}),
            ("s", 70, {"force": [69, 33]}), ("c", 4500, {}), ("c", 4500, {})]


FM_MODES = [(m, D) for m in ("both", "emb") for D in (4, 10, 16, 64)] + [("lr", 1)]


@pytest.mark.parametrize("mode,D", FM_MODES, ids=["%s-%d" % md for md in FM_MODES])
@pytest.mark.parametrize("rule", RULES)
def test_fm_both_tiers(rule, mode, D):
    """D 4 / 16 / 64: float4, G = 1 / 4 / 16; D = 10: scalar, G = 16.  "emb": lr == NULL.  "lr": emb == NULL -- one tier (B),
    D = 1, G = 1."""
    c = Fm(_fm_fields(), D, mode=mode, seed=D)
    rows = (c.emb.get("s") or c.lr.get("s")).rows.tolist()
    assert all(r in rows for r in (31, 32, 69))
    c.run("fm %s D=%d" % (mode, D), rule, zero_rows_of="a")


@pytest.mark.parametrize("D", [16, 10])
@pytest.mark.parametrize("rule", RULES)
def test_fm_frozen_embedding_with_a_trained_lr_table(rule, D):
    """emb[i].grad == NULL on a tier-A table ("a") and on a tier-B one ("b"): their LR tables are stepped, the embedding
    tables and the state passed for them are not written."""
    f = _fm_fields()
    f[0] = ("a", 37, dict(f[0][2], frozen_emb=True))
    f[2] = ("b", 5000, dict(f[2][2], frozen_emb=True))
    c = Fm(f, D, seed=21)
    c.run("fm frozen emb D=%d" % D, rule, zero_rows_of="a")


@pytest.mark.parametrize("stride", [20, 17])
@pytest.mark.parametrize("rule", RULES)
def test_fm_packed_embedding_tables(rule, stride):
    """D = 16 inside rows of 20 floats (w_stride % 4 == 0: float4) and of 17 (scalar form), on a tier-A and a tier-B table;
    gradient and state stay contiguous [V, 16]; columns 16 .. stride - 1 of the storage are not written."""
    f = _fm_fields()
    f[1] = ("s", 70, dict(f[1][2], stride=stride))
    f[4] = ("c", 4500, {"stride": stride})
    c = Fm(f, 16, seed=stride)
    c.run("fm packed stride %d" % stride, rule)


@pytest.mark.parametrize("where", ["tier A", "tier B"])
def test_fm_refusals_write_nothing(where):
    """A packed LR table (table_stride 17 on the LR descriptor) is refused with RBX_ERR_UNSUPPORTED, and a missing state
    tensor with RBX_ERR_INVALID, before anything is launched -- on a tier-A table too, which is described only after tier
    B's pairs have been walked (pin: the parent stepped tier B first and refused afterwards)."""
    from recbox_amd import _lib
    c = Fm(_fm_fields(), 16, seed=31)
    i = 0 if where == "tier A" else 2
    hp = hp_of("adam")
    c.la[i].table_stride = 17
    rc = c.update("adam", hp, 0.0)
    assert rc == _lib.RBX_ERR_UNSUPPORTED, rc
    for n, p in c.all:
        after = p.snap()
        for k in ("store", "s1", "s2", "g"):
            assert torch.equal(after[k], c.start[n][k]), "refused packed LR table (%s): %s %s was written" % (where, n, k)
    c.la[i].table_stride = 0
    keep = c.l_of[i]
    c.l_of[i] = None                                        # no state for this LR table
    rc = c.update("adam", hp, 0.0)
    c.l_of[i] = keep
    assert rc == _lib.RBX_ERR_INVALID, rc
    for n, p in c.all:
        after = p.snap()
        for k in ("store", "s1", "s2", "g"):
            assert torch.equal(after[k], c.start[n][k]), "refused missing state (%s): %s %s was written" % (where, n, k)
    assert c.update("adam", hp, 0.0) == 0                   # and the same call with everything in place is served


@pytest.mark.parametrize("D", [16, 10])
@pytest.mark.parametrize("rule", RULES)
def test_fm_second_tier_a_block(rule, D):
    """B = kTaBlock + 5 = 2053: NB = 2.  Row 60 of "s" is named by sample 2051 alone -- its bit is set only in the second
    block's bitmap; the last 8 samples (all in block 1) carry a zero gradient."""
    B = K_TA_BLOCK + 5
    c = Fm([("a", 37, {"pad": 0, "force": [0]}), ("s", 70, {"force": [31, 32, 69]}), ("b", 5000, {})], D, B=B, seed=41,
           tail_only=("s", 60))
    ids = c.keep[1].cpu().long()
    assert int((ids == 60).sum()) == 1 and int((ids == 60).nonzero()) >= K_TA_BLOCK
    assert 60 in c.emb["s"].rows.tolist()
    c.run("fm B=%d D=%d" % (B, D), rule, zero_rows_of="s")


@pytest.mark.parametrize("rule", RULES)
def test_fm_33_tier_a_tables(rule):
    """33 tables of 5 .. 36 rows, D = 4: the 33rd takes a launch of its own (kTaUpdTables = 32)."""
    c = Fm([("t%d" % i, 5 + i % 32, {"pad": 0} if i % 3 == 0 else {}) for i in range(K_TA_TABLES + 1)], 4, seed=51)
    c.run("fm 33 tier-A tables", rule)


# ======== rbx_embed_csr_sparse_update: the existing C-ABI cases, held to the oracle ==========================================
@pytest.mark.parametrize("dims", [(1, 1, 1), (10, 10, 10), (16, 16, 16), (128, 128, 128), (260, 260, 260), (67, 67, 67), (16, 10, 16)],
                         ids=lambda d: "x".join(map(str, d)))
@pytest.mark.parametrize("rule", RULES)
def test_csr_cases_of_the_earlier_file_against_the_oracle(rule, dims):
    from test_gpu_embed_csr_optim import HP, Call, _clones
    c = Call(rule, dims, seed=sum(dims))
    c.sort_and_backward()
    t0, a0, b0, g0 = _clones(c.tables), _clones(c.s1), _clones(c.s2), _clones(c.grads)
    c.update(t0, g0, a0, b0, clear=0)
    h = HP[rule]
    b1, b2 = h.get("betas", (0.0, 0.0))
    lr = h["lr"] * math.sqrt(1 - b2) / (1 - b1) if rule == "adam" else h["lr"]
    for k in range(1, len(c.names)):
        rows = c.rows[c.names[k]].cpu()
        (w, a_w), (n1, a1), (n2, a2) = O.step_rows(KIND[rule], c.tables[k], c.grads[k], rows, c.s1[k], c.s2[k], lr=lr, beta1=b1,
                                                   beta2=b2, eps=h.get("eps", 0.0))
        tag = "csr %s %s %s" % (rule, dims, c.names[k])
        check(tag + " w", t0[k], w, a_w)
        if rule != "sgd":
            check(tag + " state1", a0[k], n1, a1)
        if rule == "adam":
            check(tag + " state2", b0[k], n2, a2)


# ======== rbx_opt_advance ======================================================================================================
ADVANCE = [("adam", 0.01, 0.9, 0.999, 0.0), ("adam", 0.01, 0.5, 0.9999, 0.0), ("adam", 0.01, 0.0, 0.999, 0.0),
           ("adagrad", 0.05, 0.0, 0.0, 0.0), ("adagrad", 0.05, 0.0, 0.0, 0.1), ("sgd", 0.05, 0.0, 0.0, 0.0)]


@pytest.mark.parametrize("case", ADVANCE, ids=lambda c: "%s-%g-%g-%g" % (c[0], c[2], c[3], c[4]))
def test_opt_advance_counts_exactly_and_writes_the_step_size_of_its_step(case):
    """t = 1 .. 40 from a counter at 0, then three calls from a counter at 5000: *d_t is exact, *d_step_size within the
    relative bound K eps32 of oracle/optim64.step_size (K from the conditioning of 1 - b^t and the allowance for powf).
    Also prints the by-value step size (recbox_amd.optim._step_size, a double) against the device's."""
    from recbox_amd import optim
    from recbox_amd._lib import check as ok, lib
    rule, lr, b1, b2, dec = case
    dev = torch.zeros(2, device="cuda")
    t_dev, s_dev = dev[0:1], dev[1:2]
    by_value = {"sgd": lambda: optim.SparseSGD([dev], lr=lr), "adagrad": lambda: optim.SparseAdagrad([dev], lr=lr, lr_decay=dec),
                "adam": lambda: optim.SparseAdam([dev], lr=lr, betas=(b1, b2))}[rule]()
    worst, worst_bv = 0.0, 0.0
    try:
        for start, n in ((0, 40), (5000, 3)):
            t_dev.fill_(float(start))
            for t in range(start + 1, start + n + 1):
                ok(lib.rbx_opt_advance(KIND[rule], lr, b1, b2, dec, _ptr(t_dev), _ptr(s_dev), _stream()))
                got_t, got = [float(x) for x in dev.cpu()]
                assert got_t == float(t), (got_t, t)
                want, K = O.step_size(KIND[rule], lr, b1, b2, dec, t)
                err = abs(got - want) / (EPS32 * want)
                if K == 0.0:
                    assert got == want
                else:
                    worst = max(worst, err / K)
                    assert err <= K, "t = %d: %.2f eps32 > K = %.2f" % (t, err, K)
                worst_bv = max(worst_bv, abs(by_value._step_size(t) - got) / (EPS32 * want) / max(K, 1.0))
    finally:
        from recbox_amd import ops
        ops.config.track_touched_rows = False
    _note("opt_advance %s step size" % (case,), worst, 1.0)
    _note("opt_advance %s by-value vs device" % (case,), worst_bv, 1.0)
    print("opt_advance %s: worst err / bound %.3f; by-value vs device %.3f of the bound" % (case, worst, worst_bv))
    assert worst_bv <= 1.0, "the by-value step size is outside the bound of the device's"


@pytest.mark.parametrize("rule", RULES)
def test_device_step_size_gives_the_bits_of_the_same_value_in_lr(rule):
    """One update with d_step_size set (lr holds garbage) and one with the value rbx_opt_advance wrote passed in lr: tables
    and state bit-equal, on the padded path and on both tiers of the fused FM path."""
    from recbox_amd._lib import check as ok, lib
    hp = dict(hp_of(rule))
    dev = torch.zeros(2, device="cuda")
    dev[0] = 6.0
    ok(lib.rbx_opt_advance(KIND[rule], 0.01, hp.get("beta1", 0.0), hp.get("beta2", 0.0), 0.1, _ptr(dev[0:1]), _ptr(dev[1:2]),
                           _stream()))
    step = float(dev[1])
    assert float(dev[0]) == 7.0 and step > 0
    for c in (Embed([("a", 211, 16, {}), ("b", 211, 10, {})], seed=61), Fm(_fm_fields(), 16, seed=62)):
        c.reset()
        assert c.update(rule, dict(hp, lr=1e9), 0.05, d_step=dev[1:2]) == 0
        got = [p.snap() for p in (list(c.params.values()) if isinstance(c, Embed) else [p for _, p in c.all])]
        c.reset()
        assert c.update(rule, dict(hp, lr=step), 0.05) == 0
        want = [p.snap() for p in (list(c.params.values()) if isinstance(c, Embed) else [p for _, p in c.all])]
        for a, b in zip(got, want):
            for k in ("store", "s1", "s2"):
                assert torch.equal(a[k], b[k]), (rule, type(c).__name__, k)
        assert not torch.equal(got[0]["store"], (c.start["a"] if isinstance(c, Embed) else c.start["emb a"])["store"])


def test_opt_advance_and_updates_refuse_bad_arguments():
    from recbox_amd import _lib
    from recbox_amd._lib import lib
    dev = torch.full((2,), 3.0, device="cuda")
    for kind in (-1, 3):
        assert lib.rbx_opt_advance(kind, 0.01, 0.9, 0.999, 0.0, _ptr(dev[0:1]), _ptr(dev[1:2]), _stream()) == _lib.RBX_ERR_INVALID
    assert lib.rbx_opt_advance(O.ADAM, 0.01, 0.9, 0.999, 0.0, None, _ptr(dev[1:2]), _stream()) == _lib.RBX_ERR_INVALID
    assert lib.rbx_opt_advance(O.ADAM, 0.01, 0.9, 0.999, 0.0, _ptr(dev[0:1]), None, _stream()) == _lib.RBX_ERR_INVALID
    torch.cuda.synchronize()
    assert dev.tolist() == [3.0, 3.0]
    c = Embed([("a", 50, 16, {})], seed=71)
    opt = _opt("adam", hp_of("adam"), 0.0)
    opt.kind = 3
    arr = (ctypes.c_void_p * 1)(c.params["a"].s1.data_ptr())
    assert lib.rbx_embed_sparse_update(c.arr, 1, c.B, _ptr(c.ws), c.ws_bytes, ctypes.byref(opt), arr, arr, _stream()) == _lib.RBX_ERR_INVALID
    opt.kind = O.ADAM
    assert lib.rbx_embed_sparse_update(c.arr, 1, c.B, _ptr(c.ws), c.ws_bytes, ctypes.byref(opt), arr, None, _stream()) == _lib.RBX_ERR_INVALID
    assert lib.rbx_embed_sparse_update(c.arr, 1, c.B, _ptr(c.ws), c.ws_bytes, None, arr, arr, _stream()) == _lib.RBX_ERR_INVALID
    torch.cuda.synchronize()
    p = c.params["a"]
    assert torch.equal(p.store, c.start["a"]["store"]) and torch.equal(p.s1, c.start["a"]["s1"])


# ======== recbox_amd.optim over every kind of record ==========================================================================
def _make_opt(rule, params):
    from recbox_amd import optim
    if rule == "sgd":
        return optim.SparseSGD(params, lr=0.05, weight_decay=0.03), dict(lr=0.05)
    if rule == "adagrad":
        return (optim.SparseAdagrad(params, lr=0.05, lr_decay=0.1, eps=1e-10, weight_decay=0.03, initial_accumulator_value=0.25),
                dict(lr=0.05, lr_decay=0.1, eps=1e-10))
    return optim.SparseAdam(params, lr=0.01, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.03), dict(lr=0.01, beta1=0.9, beta2=0.999,
                                                                                                  eps=1e-8)


def _held_step(tag, rule, opt, hp, t, tables, rows_of, backward):
    """zero_grad, ``backward()``, step -- every table in ``tables`` {name: parameter} against one oracle step from its own
    previous value and state on ``rows_of[name]``."""
    opt.zero_grad()
    backward()
    before = {}
    for n, p in tables.items():
        st = opt._state_of(p)["s"]
        before[n] = (p.detach().clone(), p.grad.detach().clone(), [s.clone() for s in st])
    opt.step()
    torch.cuda.synchronize()
    lr_t, _ = O.step_size(KIND[rule], hp["lr"], hp.get("beta1", 0.0), hp.get("beta2", 0.0), hp.get("lr_decay", 0.0), t)
    worst = 0.0
    for n, p in tables.items():
        w0, g0, s0 = before[n]
        s0 = s0 + [None, None]
        (w, a_w), (n1, a1), (n2, a2) = O.step_rows(KIND[rule], w0, g0, rows_of[n], s0[0], s0[1], lr=lr_t, beta1=hp.get("beta1", 0.0),
                                                   beta2=hp.get("beta2", 0.0), eps=hp.get("eps", 0.0), weight_decay=0.03)
        st = opt._state_of(p)["s"]
        worst = max(worst, check("%s %s step %d w" % (tag, n, t), p, w, a_w))
        if rule != "sgd":
            worst = max(worst, check("%s %s step %d state1" % (tag, n, t), st[0], n1, a1))
        if rule == "adam":
            worst = max(worst, check("%s %s step %d state2" % (tag, n, t), st[1], n2, a2))
    return worst


@pytest.mark.parametrize("path", ["embed", "fm_fused", "bags", "dense"])
@pytest.mark.parametrize("rule", RULES)
def test_optimisers_through_every_record_kind(rule, path):
    """SparseSGD / SparseAdagrad / SparseAdam with weight_decay, lr_decay and initial_accumulator_value set, three steps, each
    held to the oracle from the device's own previous table and state (bounds do not compound)."""
    from recbox_amd import ops
    try:
        if path == "embed":
            from recbox_amd.rechub.basic.features import SparseFeature
            from recbox_amd.rechub.basic.layers import EmbeddingLayer
            feats = [SparseFeature("u", 503, 16), SparseFeature("i", 37, 16)]
            layer = EmbeddingLayer(feats).cuda()
            tables = dict((f.name, layer.embed_dict[f.name].weight) for f in feats)
            opt, hp = _make_opt(rule, list(tables.values()))
            for t in range(1, 4):
                gen = torch.Generator().manual_seed(300 + t)
                x = dict((f.name, torch.randint(0, f.vocab_size, (65,), generator=gen).cuda()) for f in feats)
                dY = torch.randn(65, 32, generator=gen).div_(65).cuda()
                rows = dict((n, torch.unique(v.cpu())) for n, v in x.items())
                _held_step("optim embed %s" % rule, rule, opt, hp, t, tables, rows, lambda: layer(x, feats, squeeze_dim=True).backward(dY))
            assert opt.calls["rows"] == 3 and opt.calls["dense"] == 0, opt.calls
        elif path == "bags":
            from test_gpu_embed_csr_optim import _layer, _layer_batch
            layer, feats = _layer()
            tables = dict((f.name, layer.embed_dict[f.name].weight) for f in feats)
            opt, hp = _make_opt(rule, list(tables.values()))
            for t in range(1, 4):
                x, rows, dY = _layer_batch(65, 310 + t)
                rows = dict((n, r.cpu()) for n, r in rows.items())
                _held_step("optim bags %s" % rule, rule, opt, hp, t, tables, rows, lambda: layer(x, feats, squeeze_dim=True).backward(dY))
            assert opt.calls["rows"] == 6 and opt.calls["dense"] == 0, opt.calls
        elif path == "fm_fused":
            from recbox_amd import optim
            from recbox_amd.ranking.pytorch.models import FM
            from test_gpu_ranking import _criteo_like, _cuda
            vocabs = [37, 5, 5000]
            fm, _, _ = _criteo_like(4, vocabs, 16, seed=3)
            model = FM(fm, 16, fused=True).cuda()
            with torch.no_grad():
                for p in model.parameters():
                    p.normal_(0, 0.1)
            params, rest = optim.split_parameters(model)
            feat_of = {}
            for holder in (model.embedding_layer.embedding_layer.embedding_layers,
                           model.fm.lr_layer.embedding_layer.embedding_layer.embedding_layers):
                for fname, mod in holder.items():
                    if isinstance(mod, torch.nn.Embedding):
                        feat_of[id(mod.weight)] = fname
            tables = dict(("%s/%d" % (feat_of[id(p)], p.shape[1]), p) for p in params)
            assert len(tables) == 6
            opt, hp = _make_opt(rule, params)
            for t in range(1, 4):
                _, X, y = _criteo_like(65, vocabs, 16, seed=320 + t)
                Xc, yc = _cuda(X), y.cuda()
                rows = dict((n, torch.unique(X[n.split("/")[0]].long())) for n in tables)      # (ids >= 1: padding row 0 is not named)

                def backward():
                    for p in rest:
                        p.grad = None
                    torch.nn.functional.binary_cross_entropy(torch.sigmoid(model.logits(Xc)), yc, reduction="mean").backward()
                _held_step("optim fm_fused %s" % rule, rule, opt, hp, t, tables, rows, backward)
            assert opt.calls["rows"] == 3 and opt.calls["dense"] == 0, opt.calls
        else:
            from recbox_amd import optim
            gen = torch.Generator().manual_seed(330)
            p = torch.nn.Parameter(torch.randn(97, 16, generator=gen).mul_(0.1).cuda())
            tables = {"p": p}
            opt, hp = _make_opt(rule, [p])
            for t in range(1, 4):
                rows = torch.randperm(97, generator=gen)[:40]
                g = torch.zeros(97, 16)
                g[rows] = torch.randn(40, 16, generator=gen).div_(65)
                assert bool((g[rows] != 0).any(dim=1).all())          # the fallback selects rows by g != 0: give every row one

                def backward():
                    p.grad = g.cuda()
                _held_step("optim dense %s" % rule, rule, opt, hp, t, tables, {"p": rows}, backward)
            assert opt.calls["dense"] == 3 and opt.calls["rows"] == 0, opt.calls
    finally:
        ops.config.track_touched_rows = False
