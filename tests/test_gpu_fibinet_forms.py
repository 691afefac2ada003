"""The SENET gate and the bilinear pair op (``ops.senet_gate`` / ``ops.bilinear_pairs``, csrc/rbx_bilinear.hip) at every form the
host side of the launches can select, against the float64 restatement of tests/fibinet64.py under the scale-aware bar of
tests/fp32_bar.py: per tensor max|got - want| <= max(4 e32, 2e-6 max|want|), e32 the error of the same restatement run in fp32
on the CPU.  Every name of ``fibinet64.NAMES`` is held to it in every case; the compositions are patched to fail, so a fall-back
cannot pass.  tests/test_gpu_fibinet.py stops at F = 26 and B = 257; the forms below lie beyond it.

The host-side quantities, restated here from the .hip file (``forms``; P = F (F - 1) / 2, tiles = ceil(B / 16)):
  forward   split = max(1, min(8, ceil(1024 / tiles), (P + 3) / 4)), ppb = ceil(P / split) pairs per blockIdx.y, ylast = the
            pairs of the last blockIdx.y; LDS = 4 (16 S + 16 (F + 1)) bytes, S = F D rounded up to 64, + 4
  dx        LDS = the forward's + 4 (64 (D + 1) + 64); above 64 KiB a kernel has to be opted in (allow_lds)
  dW        NP = 4 (D = 32) or 8 pairs per wavefront, groups = ceil(P / 4 NP), want = clamp(512 / groups, 1, tiles),
            tpc = ceil(tiles / want) tiles per chunk, chunks = ceil(tiles / tpc), clast = the tiles of the last chunk
  gate      forward grid = min(ceil(B / 4), 1024) workgroups of 4 samples, ftrips = trips of workgroup 0; backward grid =
            min(ceil(B / 4), 256), per = ceil(B / grid) samples per workgroup, btrips = ceil(per / 4)
``chunks`` and the gate's backward grid are also read from the library (the workspace-size entry points) and must agree.

  case          B      F   D   R  kind / layout / scale / act        what it selects                          form reached
  lds-64x32     17     64  32  21 interaction io plain relu          fwd 135 488 B, dx 144 192 B              both opt-ins, the widest shape
  lds-64x16     17     64  16  21 each        oi scale sigmoid       fwd 69 952 B, dx 74 560 B                both opt-ins, da at F = 64
  lds-30x32     17     30  32  10 all         io scale relu          fwd 63 680 B, dx 72 384 B                only the backward opts in
  p-63x8        17     63  8   21 interaction oi scale relu          P = 1953 = 61 x 32 + 1, ppb 245, ylast 238  pair tails of dW (4 NP = 32) and fwd
  tpc2-26x16    771    26  16  8  each        io scale relu          groups 11, tiles 49, tpc 2, chunks 25, clast 1 (3 rows)  the tile loop of bl_dw_kernel
  tpc2-64x32    81     64  32  21 interaction oi plain sigmoid       groups 126, tiles 6, tpc 2, chunks 3     the tile loop with NP = 4, LDS opt-in
  tpc3-45x4     533    45  4   15 all         oi scale sigmoid       groups 31, tiles 34, tpc 3, chunks 12, clast 1  three trips, NP = 8 at D = 4
  split1-3x4    16385  3   4   1  interaction io scale relu          tiles 1025, split 1; tpc 3, chunks 342, clast 2; gate ftrips 5, btrips 17, R = 1
  split1-5x4    16385  5   4   1  each        oi plain sigmoid       ceil(1024 / tiles) = 1 < (P + 3) / 4 = 3: the batch, not P, makes split 1
  split4-7x8    4101   7   8   2  all         io scale relu          tiles 257, split 4, ppb 6, ylast 3; gate ftrips 2, btrips 5 (per 17)
  gate-1029     1029   3   4   32 all         io scale relu          gate backward per 5: trips of 4 + 1 samples; R = 32 = kGateMaxR
(At F = 3 the pair clamp (P + 3) / 4 = 1 already gives split 1 at every batch, so split1-5x4 is the case where 1025 tiles decide.)
Beside them: R = 33 and F = 65 are refused and run the composition (the forward bit for bit, the gradients under the bar); an
empty batch; run-to-run bits at tpc2-26x16 and gate-1029.

Inputs: ``fibinet64.make_case`` redraws the samples whose ReLU pre-activation lies within KINK = 1e-3 of the layer's largest
magnitude of zero and refuses a seed that still has one, so every case here keeps ``kink_margin`` above KINK at unit scale --
no weight had to be widened; tests/test_fibinet_host.py asserts it for this list on the CPU, and that the fp32 restatement and
the fp32 composition hold the bar before anything runs on a GPU.

No figure of this module had been measured on a GPU when it was written.  Measured on the MI355X afterwards, worst err / bar
over the module (18 tests, 4 s): out 0.165, a 0.231, dx 0.246, dscale 0.174, dW 0.213, dw1 0.237, dw2 0.255 -- every kernel holds
the bar on every form and none had to be changed.  Mutation check (scratch builds, never committed; wrong numbers only, in bounds,
terminating), this module / tests/test_gpu_fibinet.py: bl_dw_kernel re-reading its chunk's first tile on every trip 5 failed / 34
passed; bl_fwd_kernel placing blockIdx.y at (P + 7) / 8 pairs whenever ppb > 4 (right for a split of 8) 1 failed (split4-7x8) / 34
passed; gate_bwd_kernel re-reading its first four samples on every trip 4 failed / 34 passed.  profiles/fibinet/INDEX.md quotes
the same."""
import os
import re

import pytest
import torch

import fibinet64
import fp32_bar

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_OPT_IN = 64 * 1024

# name -> (B, F, D, R, kind, transposed, with_scale, act), and what the case has to reach (keys of ``forms``)
CASES = {
    "lds-64x32": ((17, 64, 32, 21, "field_interaction", False, False, "relu"),
                  {"fwd_lds": 135488, "dx_lds": 144192, "tiles": 2, "split": 8, "ppb": 252}),
    "lds-64x16": ((17, 64, 16, 21, "field_each", True, True, "sigmoid"), {"fwd_lds": 69952, "dx_lds": 74560}),
    "lds-30x32": ((17, 30, 32, 10, "field_all", False, True, "relu"), {"fwd_lds": 63680, "dx_lds": 72384, "ppb": 55, "ylast": 50}),
    "p-63x8": ((17, 63, 8, 21, "field_interaction", True, True, "relu"), {"P": 1953, "groups": 62, "ppb": 245, "ylast": 238}),
    "tpc2-26x16": ((771, 26, 16, 8, "field_each", False, True, "relu"),
                   {"groups": 11, "want": 46, "tiles": 49, "tpc": 2, "chunks": 25, "clast": 1}),
    "tpc2-64x32": ((81, 64, 32, 21, "field_interaction", True, False, "sigmoid"),
                   {"groups": 126, "want": 4, "tiles": 6, "tpc": 2, "chunks": 3, "dx_lds": 144192}),
    "tpc3-45x4": ((533, 45, 4, 15, "field_all", True, True, "sigmoid"),
                  {"groups": 31, "want": 16, "tiles": 34, "tpc": 3, "chunks": 12, "clast": 1}),
    "split1-3x4": ((16385, 3, 4, 1, "field_interaction", False, True, "relu"),
                   {"tiles": 1025, "split": 1, "ppb": 3, "tpc": 3, "chunks": 342, "clast": 2, "gate_fwd_grid": 1024, "ftrips": 5,
                    "gate_bwd_grid": 256, "per": 65, "btrips": 17}),
    "split1-5x4": ((16385, 5, 4, 1, "field_each", True, False, "sigmoid"),
                   {"tiles": 1025, "split_by_tiles": 1, "split_by_pairs": 3, "split": 1, "ppb": 10}),
    "split4-7x8": ((4101, 7, 8, 2, "field_all", False, True, "relu"),
                   {"tiles": 257, "split": 4, "ppb": 6, "ylast": 3, "gate_fwd_grid": 1024, "ftrips": 2, "per": 17, "btrips": 5}),
    "gate-1029": ((1029, 3, 4, 32, "field_all", False, True, "relu"), {"gate_bwd_grid": 256, "per": 5, "btrips": 2, "ftrips": 1}),
}
BITS = ("tpc2-26x16", "gate-1029")
_CACHE = {}


# ---- the launch geometry, restated ---------------------------------------------------------------------------------------------
def _ceil(a, b):
    return -(-a // b)


def constants():
    """The constants of csrc/rbx_bilinear.hip the restatement depends on, read from the source; the two literals of the
    forward's split are held to their lines."""
    with open(os.path.join(ROOT, "recbox_amd", "csrc", "rbx_bilinear.hip")) as fh:
        text = fh.read()
    k = {name: int(re.search(r"\b%s = (\d+)" % name, text).group(1))
         for name in ("kBlMaxF", "kBlTile", "kBlDwBlocks", "kGateMaxR", "kGateFwdGrid", "kGateBwdGrid")}
    assert "long long split = (1024 + tiles - 1) / tiles;" in text and "if (split > 8) split = 8;" in text
    assert "if (split > (P + 3) / 4) split = (P + 3) / 4;" in text and "static constexpr int NP = D == 32 ? 4 : 8;" in text
    assert "return ((fd + 63) / 64) * 64 + 4;" in text
    return k


def forms(B, F, D, R, k=None):
    """Every host-side quantity of the four launches for one shape (see the module's docstring)."""
    k = k or constants()
    P, tiles = F * (F - 1) // 2, _ceil(B, k["kBlTile"])
    q = {"P": P, "tiles": tiles, "split_by_tiles": _ceil(1024, tiles), "split_by_pairs": (P + 3) // 4}
    q["split"] = max(1, min(8, q["split_by_tiles"], q["split_by_pairs"]))
    q["ppb"] = _ceil(P, q["split"])
    q["yblocks"] = _ceil(P, q["ppb"])
    q["ylast"] = P - (q["yblocks"] - 1) * q["ppb"]
    stride = _ceil(F * D, 64) * 64 + 4
    q["fwd_lds"] = 4 * (k["kBlTile"] * stride + k["kBlTile"] * (F + 1))
    q["dx_lds"] = q["fwd_lds"] + 4 * (4 * k["kBlTile"] * (D + 1) + 4 * k["kBlTile"])
    np_ = 4 if D == 32 else 8
    q["groups"] = _ceil(P, 4 * np_)
    q["want"] = min(max(1, k["kBlDwBlocks"] // q["groups"]), tiles)
    q["tpc"] = _ceil(tiles, q["want"])
    q["chunks"] = _ceil(tiles, q["tpc"])
    q["clast"] = tiles - (q["chunks"] - 1) * q["tpc"]
    q["gate_fwd_grid"] = min(_ceil(B, 4), k["kGateFwdGrid"])
    q["ftrips"] = _ceil(_ceil(B, 4), q["gate_fwd_grid"])
    q["gate_bwd_grid"] = min(_ceil(B, 4), k["kGateBwdGrid"])
    q["per"] = _ceil(B, q["gate_bwd_grid"])
    q["btrips"] = _ceil(q["per"], 4)
    return q


def check_forms(name):
    """The case reaches what the table says it reaches; the chunk count and the gate's grid agree with the library's."""
    from recbox_amd import _lib
    (B, F, D, R, _, _, _, _), expect = CASES[name]
    q = forms(B, F, D, R)
    for key, value in expect.items():
        assert q[key] == value, "%s: %s is %d, the table says %d" % (name, key, q[key], value)
    lib = _lib.lib
    assert lib.rbx_bilinear_pairs_supported(F, D, _lib.RBX_F32) == 1 and lib.rbx_senet_gate_supported(F, D, R, _lib.RBX_F32) == 1
    assert lib.rbx_bilinear_pairs_bwd_workspace_size(B, F, D) == 4 * q["chunks"] * q["P"] * D * D, name
    assert lib.rbx_senet_gate_bwd_workspace_size(B, F, R) == 8 * q["gate_bwd_grid"] * F * R, name
    return q


def check_the_list_covers_every_form():
    """Over the whole list: each direction of the LDS opt-in on both sides of 64 KiB, tpc of 1, 2 and 3 with a short last chunk,
    split of 1, between 2 and 7 with a short last blockIdx.y, and 8, both gate loops, R of 1 and kGateMaxR."""
    k = constants()
    qs = {name: forms(*CASES[name][0][:4], k=k) for name in CASES}
    assert k["kBlMaxF"] == 64 and k["kGateMaxR"] == 32
    assert qs["lds-64x32"]["fwd_lds"] > LDS_OPT_IN and qs["lds-64x16"]["fwd_lds"] > LDS_OPT_IN
    assert qs["lds-30x32"]["fwd_lds"] < LDS_OPT_IN < qs["lds-30x32"]["dx_lds"]
    assert all(q["dx_lds"] <= 160 * 1024 for q in qs.values())
    assert qs["p-63x8"]["P"] % 32 != 0 and qs["p-63x8"]["P"] % qs["p-63x8"]["ppb"] != 0
    assert {q["tpc"] for q in qs.values()} >= {1, 2, 3}
    assert any(q["tpc"] > 1 and q["clast"] < q["tpc"] for q in qs.values())
    assert {q["split"] for q in qs.values()} >= {1, 4, 8}
    assert 1 < qs["split4-7x8"]["split"] < 8 and qs["split4-7x8"]["ylast"] < qs["split4-7x8"]["ppb"]
    assert qs["split1-5x4"]["split_by_tiles"] < qs["split1-5x4"]["split_by_pairs"]
    assert qs["gate-1029"]["per"] % 4 != 0 and qs["gate-1029"]["btrips"] == 2
    assert max(q["ftrips"] for q in qs.values()) > 1
    assert {c[0][3] for c in CASES.values()} >= {1, k["kGateMaxR"]}
    assert {c[0][4] for c in CASES.values()} == set(fibinet64.KINDS) and {c[0][5] for c in CASES.values()} == {True, False}
    assert {c[0][6] for c in CASES.values()} == {True, False} and {c[0][7] for c in CASES.values()} == {"relu", "sigmoid"}


def make(name, seed=11):
    B, F, D, R, kind, tr, _, act = CASES[name][0]
    return fibinet64.make_case(seed, B, F, D, kind, R=R, act=act, transposed=tr)


def _case(name):
    """(case, (float64, fp32 on the CPU)) of a case, computed once."""
    if name not in _CACHE:
        case, ws = make(name), CASES[name][0][6]
        _CACHE[name] = (case, (fibinet64.reference(case, ws), fibinet64.reference(case, ws, torch.float32)))
    return _CACHE[name]


# ---- the tests -----------------------------------------------------------------------------------------------------------------
@pytest.fixture
def fused_only(monkeypatch):
    from recbox_amd import ops
    monkeypatch.setattr(ops.config, "bilinear_fused", True)
    monkeypatch.setattr(ops, "bilinear_pairs_torch", lambda *a, **k: pytest.fail("the fused pair op did not run"))
    monkeypatch.setattr(ops, "senet_gate_torch", lambda *a, **k: pytest.fail("the fused gate did not run"))


def _assert_all(tag, got, refs):
    want, ref32 = refs
    for name in fibinet64.NAMES:
        fp32_bar.assert_bar("%s %s" % (name, tag), got[name], want[name], ref32[name])


def _run(name):
    from recbox_amd import ops
    return fibinet64.run(ops.senet_gate, ops.bilinear_pairs, _case(name)[0], "cuda", CASES[name][0][6])


def test_the_list_covers_every_form():
    check_the_list_covers_every_form()


@pytest.mark.parametrize("name", list(CASES))
def test_form_matches_float64_under_the_fp32_bar(name, fused_only):
    q = check_forms(name)
    print("%s: %s" % (name, ", ".join("%s %d" % kv for kv in sorted(q.items()))))
    _assert_all(name, _run(name), _case(name)[1])


@pytest.mark.parametrize("name", BITS)
def test_two_runs_give_the_same_bits(name, fused_only):
    q = check_forms(name)
    assert q["tpc"] > 1 or q["btrips"] > 1
    first, second = _run(name), _run(name)
    for key in fibinet64.NAMES:
        assert torch.equal(first[key], second[key]), (name, key)


class _Calls(object):
    """Counts the calls of a function and passes them on."""

    def __init__(self, real):
        self.real, self.hits = real, 0

    def __call__(self, *a, **k):
        self.hits += 1
        return self.real(*a, **k)


@pytest.mark.parametrize("B,F,D,R,refuses", [(9, 5, 8, 33, "gate"), (9, 65, 4, 21, "both")])
def test_refused_shapes_return_the_bits_of_the_composition(B, F, D, R, refuses, monkeypatch):
    """R = 33 (the gate alone) and F = 65 (both ops): the forward is the composition's, bit for bit; the gradients hold the bar
    (the composition's index backward adds with atomics, so its gradients have no fixed bits to compare with)."""
    from recbox_amd import _lib, ops
    assert _lib.lib.rbx_senet_gate_supported(F, D, R, _lib.RBX_F32) == 0
    assert _lib.lib.rbx_bilinear_pairs_supported(F, D, _lib.RBX_F32) == (0 if refuses == "both" else 1)
    case = fibinet64.make_case(5, B, F, D, "field_each", R=R)
    refs = (fibinet64.reference(case), fibinet64.reference(case, True, torch.float32))
    plain = fibinet64.run(ops.senet_gate_torch, ops.bilinear_pairs_torch, case, "cuda", True)
    gate_node, pair_node = _Calls(ops._SenetGate.apply), _Calls(ops._BilinearPairs.apply)
    gate_torch, pair_torch = _Calls(ops.senet_gate_torch), _Calls(ops.bilinear_pairs_torch)
    monkeypatch.setattr(ops._SenetGate, "apply", gate_node)
    monkeypatch.setattr(ops._BilinearPairs, "apply", pair_node)
    monkeypatch.setattr(ops, "senet_gate_torch", gate_torch)
    monkeypatch.setattr(ops, "bilinear_pairs_torch", pair_torch)
    got = fibinet64.run(ops.senet_gate, ops.bilinear_pairs, case, "cuda", True)
    assert gate_node.hits == 0 and gate_torch.hits == 1
    assert (pair_node.hits, pair_torch.hits) == ((0, 1) if refuses == "both" else (1, 0))
    assert torch.equal(got["a"], plain["a"])
    if refuses == "both":
        assert torch.equal(got["out"], plain["out"])
    _assert_all("refused R=%d F=%d" % (R, F), got, refs)


def test_empty_batch():
    """B = 0 through the ops: empty results of the right shape, weight gradients that are zeros of the right shape; the C
    entries return RBX_OK before they look at a pointer."""
    from recbox_amd import _lib, ops
    F, D, R, P = 5, 8, 2, 10
    g = torch.Generator().manual_seed(1)
    x = torch.zeros(0, F, D, device="cuda", requires_grad=True)
    w1, w2, W = (torch.randn(s, generator=g).cuda().requires_grad_() for s in ((R, F), (F, R), (P, D, D)))
    a = ops.senet_gate(x, w1, w2)
    out = ops.bilinear_pairs(x, W, "field_interaction", False, a)
    assert tuple(a.shape) == (0, F) and tuple(out.shape) == (0, 2 * P, D) and tuple(ops.bilinear_pairs(x, W, "field_interaction").shape) == (0, P, D)
    (out.sum() + a.sum()).backward()
    torch.cuda.synchronize()
    for t in (x, w1, w2, W):
        assert t.grad is not None and t.grad.shape == t.shape and float(t.grad.abs().sum()) == 0.0
    lib, p = _lib.lib, W.data_ptr()
    assert lib.rbx_senet_gate_fwd(p, F * D, D, p, p, 0, F, D, R, 0, _lib.RBX_F32, p, p, None) == _lib.RBX_OK
    assert lib.rbx_senet_gate_bwd(p, p, F * D, D, p, p, p, p, 0, F, D, R, 0, _lib.RBX_F32, 0, p, p, p, p, 0, None) == _lib.RBX_OK
    assert lib.rbx_bilinear_pairs_fwd(p, F * D, D, p, None, 0, F, D, 2, 0, _lib.RBX_F32, p, P * D, None) == _lib.RBX_OK
    assert lib.rbx_bilinear_pairs_bwd(p, P * D, p, F * D, D, p, None, 0, F, D, 2, 0, _lib.RBX_F32, p, None, p, p, 0, None) == _lib.RBX_OK
    torch.cuda.synchronize()


def test_report_worst_ratio():
    """Prints the worst err / bar per tensor over this module."""
    fp32_bar.report("fibinet forms")
