"""DCN-V2's cross expert mixture (``ops.cross_mix``, csrc/rbx_crossmix.hip) at every form the host side of the launches can
select, against the float64 restatement of tests/crossmix64.py under the scale-aware bar of tests/fp32_bar.py: per tensor
max|got - want| <= max(4 e32, 2e-6 max|want|), e32 the error of the same restatement run in fp32 on the CPU.  Every name of
``crossmix64.names(L)`` is held to it in every case; the composition is patched to fail, so a fall-back cannot pass.
tests/test_gpu_crossmix.py runs the ranks {4, 8, 32, 64}, n of 3 .. 416 and at most 257 rows; the forms below lie beyond it.

The host-side quantities, restated here from the .hip file (``forms``):
  rsh = log2 r (the kernels split a column c of [E r] as expert c >> rsh, rank c & (r - 1)); ksteps = ceil(n / 4) MFMA steps
  xs = n rounded up to 4, + 4; hs = E r + 4; LDS forward 4 (16 (xs + 2 hs) + 128), backward 4 (16 (2 xs + 4 hs) + 256) bytes;
  above 64 KiB a kernel has to be opted in (allow_lds), and rbx_crossmix_supported caps the backward at 160 KiB
  rpc = ceil(B / 16) rounded up to 64 rows per chunk of the weight-gradient sums, chunks = ceil(B / rpc), clast = the rows of
  the last chunk
The workspace the library asks for (4 (B (4 E r + E) + 16 max(n E r, E r r, E n)) bytes) must agree with the restatement.

  case     B     n    r   E  L   what it selects                                     form reached
  r16-a    17    40   16  3  2   rsh 4, E r = 48 (3 column blocks + the gate's)      rank 16, two layers
  r16-b    33    17   16  8  1   rsh 4, E r = 128                                    rank 16 with 8 experts
  rpc128   1025  17   8   2  3   rpc 128, chunks 9, clast 1                          two k-loops of 64 rows per chunk, a chunk of one row,
                                                                                     dG and dx0 added up over three layers
  widest   17    640  32  8  1   fwd 75 008 B, bwd 150 016 B, ksteps 160             the largest supported shape, both opt-ins
  n637     17    637  64  4  1   xs 644 as at n = 640, ksteps 160, rsh 6             n no multiple of 4 at the top, zero padding of 3
  n1       17    1    4   1  2   ksteps 1, xs 8                                      below one k-step, one column
  n2       33    2    8   2  1   ksteps 1, xs 8                                      below one k-step
Beside them: n = 641, E = 9 and E r = 512 are refused and run the composition (the forward bit for bit, the gradients under the
bar); an empty batch; run-to-run bits at rpc128.

Inputs: ``crossmix64.make_case`` at unit scale; tests/test_crossmix_host.py asserts on the CPU that every tanh input of this
list is finite, that fewer than half of them lie in the saturated branch (|.| > 3) and that the branch is reached, and that the
fp32 restatement and the fp32 composition hold the bar before anything runs on a GPU.

No figure of this module had been measured on a GPU when it was written.  Measured on the MI355X afterwards, worst err / bar
over the module (14 tests, 3 s): out 0.213, dx0 0.142, dG 0.369, dU 0.313, dV 0.396, dC 0.371, db 0.265 (each the worst layer) --
every kernel holds the bar on every form and none had to be changed.  Mutation check (a scratch build, never committed; wrong
numbers only, in bounds): cm_fwd_kernel taking the expert of a column as (c >> 3) % E at r = 16 fails r16-a and r16-b here while
all 22 tests of tests/test_gpu_crossmix.py pass.  profiles/crossmix/INDEX.md quotes the same."""
import os
import re

import pytest
import torch

import crossmix64
import fp32_bar

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_OPT_IN = 64 * 1024

# name -> (B, n, r, E, L), and what the case has to reach (keys of ``forms``)
CASES = {
    "r16-a": ((17, 40, 16, 3, 2), {"rsh": 4, "er": 48}),
    "r16-b": ((33, 17, 16, 8, 1), {"rsh": 4, "er": 128}),
    "rpc128": ((1025, 17, 8, 2, 3), {"rpc": 128, "chunks": 9, "clast": 1}),
    "widest": ((17, 640, 32, 8, 1), {"fwd_lds": 75008, "bwd_lds": 150016, "er": 256, "ksteps": 160}),
    "n637": ((17, 637, 64, 4, 1), {"xs": 644, "bwd_lds": 150016, "ksteps": 160, "rsh": 6}),
    "n1": ((17, 1, 4, 1, 2), {"ksteps": 1, "xs": 8}),
    "n2": ((33, 2, 8, 2, 1), {"ksteps": 1, "xs": 8}),
}
REFUSED = [(9, 641, 8, 2, 1), (9, 17, 4, 9, 2), (9, 17, 64, 8, 1)]           # n = 641, E = 9, E r = 512
BITS = "rpc128"
_CACHE = {}


# ---- the launch geometry, restated ---------------------------------------------------------------------------------------------
def _ceil(a, b):
    return -(-a // b)


def constants():
    """The constants of csrc/rbx_crossmix.hip the restatement depends on, read from the source."""
    with open(os.path.join(ROOT, "recbox_amd", "csrc", "rbx_crossmix.hip")) as fh:
        text = fh.read()
    k = {name: int(re.search(r"\b%s = (\d+)" % name, text).group(1))
         for name in ("kCmTile", "kCmMaxN", "kCmMaxE", "kCmMaxER", "kCmChunks")}
    k["kCmLdsCap"] = int(re.search(r"kCmLdsCap = (\d+) \* 1024;", text).group(1)) * 1024
    assert "return ((n + 3) & ~3) + 4;" in text and "return er + 4;" in text and "per = (per + 63) / 64 * 64;" in text
    return k


def forms(B, n, r, E, L, k=None):
    """Every host-side quantity of the launches of one layer for one shape (see the module's docstring)."""
    k = k or constants()
    er, tile = E * r, k["kCmTile"]
    q = {"er": er, "rsh": r.bit_length() - 1, "tiles": _ceil(B, tile), "ksteps": _ceil(n, 4), "xs": _ceil(n, 4) * 4 + 4, "hs": er + 4}
    q["fwd_lds"] = 4 * (tile * (q["xs"] + 2 * q["hs"]) + tile * k["kCmMaxE"])
    q["bwd_lds"] = 4 * (tile * (2 * q["xs"] + 4 * q["hs"]) + 2 * tile * k["kCmMaxE"])
    q["rpc"] = _ceil(_ceil(B, k["kCmChunks"]), 64) * 64
    q["chunks"] = _ceil(B, q["rpc"])
    q["clast"] = B - (q["chunks"] - 1) * q["rpc"]
    q["workspace"] = 4 * (B * (4 * er + E) + k["kCmChunks"] * max(n * er, er * r, E * n))
    return q


def check_forms(name):
    """The case reaches what the table says it reaches, the library takes it and asks for the restated workspace."""
    from recbox_amd import _lib
    (B, n, r, E, L), expect = CASES[name]
    q = forms(B, n, r, E, L)
    for key, value in expect.items():
        assert q[key] == value, "%s: %s is %d, the table says %d" % (name, key, q[key], value)
    assert 1 << q["rsh"] == r
    assert _lib.lib.rbx_crossmix_supported(n, E, r, _lib.RBX_F32) == 1, name
    assert _lib.lib.rbx_crossmix_bwd_workspace_size(B, n, E, r) == q["workspace"], name
    return q


def check_the_list_covers_every_form():
    """Over the whole list: rank 16, more than 64 rows per chunk with a short last chunk, the widest shape on both sides of the
    forward's opt-in and under the cap, n below one k-step and n no multiple of 4, L above 1 where sums are added up."""
    k = constants()
    qs = {name: forms(*CASES[name][0], k=k) for name in CASES}
    assert (k["kCmMaxN"], k["kCmMaxE"], k["kCmMaxER"], k["kCmLdsCap"]) == (640, 8, 256, 160 * 1024)
    assert sum(1 for c in CASES.values() if c[0][2] == 16) == 2
    assert qs["rpc128"]["rpc"] > 64 and qs["rpc128"]["clast"] < 4 and CASES["rpc128"][0][4] == 3
    assert qs["widest"]["fwd_lds"] > LDS_OPT_IN and qs["widest"]["bwd_lds"] <= k["kCmLdsCap"]
    assert CASES["widest"][0][1] == k["kCmMaxN"] and qs["widest"]["er"] == k["kCmMaxER"] and CASES["widest"][0][3] == k["kCmMaxE"]
    assert CASES["n637"][0][1] % 4 != 0 and qs["n637"]["xs"] == qs["widest"]["xs"]
    assert {CASES[c][0][1] for c in ("n1", "n2")} == {1, 2}
    assert all(q["bwd_lds"] <= k["kCmLdsCap"] for q in qs.values())


def make(name, seed=11):
    B, n, r, E, L = CASES[name][0]
    return crossmix64.make_case(seed, B, n, E, r, L)


def _case(name):
    """(case, (float64, fp32 on the CPU)) of a case, computed once."""
    if name not in _CACHE:
        case = make(name)
        _CACHE[name] = (case, (crossmix64.reference(case), crossmix64.reference(case, torch.float32)))
    return _CACHE[name]


# ---- the tests -----------------------------------------------------------------------------------------------------------------
@pytest.fixture
def fused_only(monkeypatch):
    from recbox_amd import ops
    monkeypatch.setattr(ops.config, "crossmix_fused", True)
    monkeypatch.setattr(ops, "cross_mix_torch", lambda *a, **k: pytest.fail("the fused cross mixture did not run"))


def _assert_all(tag, got, refs, L):
    want, ref32 = refs
    for name in crossmix64.names(L):
        fp32_bar.assert_bar("%s %s" % (name, tag), got[name], want[name], ref32[name])


def _run(name):
    from recbox_amd import ops
    return crossmix64.run(ops.cross_mix, _case(name)[0], "cuda")


def test_the_list_covers_every_form():
    check_the_list_covers_every_form()


@pytest.mark.parametrize("name", list(CASES))
def test_form_matches_float64_under_the_fp32_bar(name, fused_only):
    q = check_forms(name)
    print("%s: %s" % (name, ", ".join("%s %d" % kv for kv in sorted(q.items()))))
    _assert_all(name, _run(name), _case(name)[1], CASES[name][0][4])


def test_two_runs_give_the_same_bits(fused_only):
    assert check_forms(BITS)["rpc"] > 64
    first, second = _run(BITS), _run(BITS)
    for key in crossmix64.names(CASES[BITS][0][4]):
        assert torch.equal(first[key], second[key]), key


class _Calls(object):
    """Counts the calls of a function and passes them on."""

    def __init__(self, real):
        self.real, self.hits = real, 0

    def __call__(self, *a, **k):
        self.hits += 1
        return self.real(*a, **k)


@pytest.mark.parametrize("shape", REFUSED, ids=lambda s: "B%d-n%d-r%d-E%d-L%d" % s)
def test_refused_shapes_return_the_bits_of_the_composition(shape, monkeypatch):
    """n = 641, E = 9 and E r = 512: the forward is the composition's, bit for bit, and the gradients hold the bar."""
    from recbox_amd import _lib, ops
    B, n, r, E, L = shape
    assert _lib.lib.rbx_crossmix_supported(n, E, r, _lib.RBX_F32) == 0
    case = crossmix64.make_case(5, B, n, E, r, L)
    refs = (crossmix64.reference(case), crossmix64.reference(case, torch.float32))
    plain = crossmix64.run(ops.cross_mix_torch, case, "cuda")
    node, composition = _Calls(ops._CrossMix.apply), _Calls(ops.cross_mix_torch)
    monkeypatch.setattr(ops._CrossMix, "apply", node)
    monkeypatch.setattr(ops, "cross_mix_torch", composition)
    got = crossmix64.run(ops.cross_mix, case, "cuda")
    assert (node.hits, composition.hits) == (0, 1)
    assert torch.equal(got["out"], plain["out"])
    _assert_all("refused %s" % (shape,), got, refs, L)


def test_empty_batch():
    """B = 0 through the op: an empty result of the right shape, weight gradients that are zeros of the right shape; the C
    entries return RBX_OK before they look at a pointer."""
    from recbox_amd import _lib, ops
    n, E, r, L = 17, 2, 8, 2
    case = crossmix64.make_case(1, 4, n, E, r, L)
    leaf = lambda t: t.detach().clone().cuda().requires_grad_()                   # noqa: E731
    x0, G = leaf(case["x0"][:0]), leaf(case["G"])
    U, V, C, b = ([leaf(t) for t in case[k]] for k in ("U", "V", "C", "b"))
    out = ops.cross_mix(x0, U, V, C, G, b)
    assert tuple(out.shape) == (0, n)
    out.sum().backward()
    torch.cuda.synchronize()
    for t in [x0, G] + U + V + C + b:
        assert t.grad is not None and t.grad.shape == t.shape and float(t.grad.abs().sum()) == 0.0
    lib, p = _lib.lib, G.data_ptr()
    assert lib.rbx_crossmix_fwd(p, n, p, n, p, p, p, p, p, 0, n, E, r, _lib.RBX_F32, p, n, None) == _lib.RBX_OK
    assert lib.rbx_crossmix_bwd(p, n, p, n, p, n, p, p, p, p, p, 0, n, E, r, _lib.RBX_F32, 0, p, n, p, n, p, p, p, p, p, p, 0,
                                None) == _lib.RBX_OK
    torch.cuda.synchronize()


def test_report_worst_ratio():
    """Prints the worst err / bar per tensor over this module."""
    fp32_bar.report("crossmix forms")
