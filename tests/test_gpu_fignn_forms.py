"""FiGNN's message-passing step (``ops.fignn_step``, csrc/rbx_fignn.hip) at every width and launch form its host side can select,
against the float64 restatement of tests/fignn64.py under the bar of tests/fp32_bar.py: per tensor
max|got - want| <= max(4 e32, 2e-6 max|want|), e32 the error of the same restatement run in fp32 on the CPU.  Every name of
``fignn64.NAMES`` is held to it in every case; the composition is patched to fail and the C forward entry is counted, so a
fall-back cannot pass.  tests/test_gpu_fignn.py runs A in {4, 8, 12, 16, 32} only, never a forward with fewer than 4 wavefronts
or a lone backward wavefront on tiles of 16, and at most 35 tiles; the forms below lie beyond it.

The host-side quantities, restated here from the .hip file (``forms``; FP = F rounded up to 16):
  scratch  = max(FP (FP + 4), 16 x 2 (A + 4)) floats per wavefront forward, max(FP (FP + 4), 16 (3 (A + 4) + 2 (3 A + 4))) backward
  LDS      = 4 (2 F T (A + 4) + 4 F T + nw scratch) bytes, opted in above 64 KiB
  T        = 16 samples to a tile where the backward with ONE wavefront fits kFgLdsCap, else 8
  nw       = the larger of 4 and 2 whose LDS fits, else 1, for each direction
  tiles    = ceil(B / T); grid = min((tiles + 1) / 2, kFgMaxGrid); trips = ceil(tiles / grid) of workgroup 0; last = the samples
             of the last tile; rows1 = grid, rows2 = grid nw_bwd: the rows of the workspace's two parts (the library's
             workspace size must agree)
  NE       = 1 up to A = 16, else 2: the N tiles of every per-field product; at A = 20, 24, 28 the second one is partial

  case     B     F   A   same  graph  T   nw f/b  LDS fwd / bwd      tiles  grid  trips  last  rows1 / 2   what it is here for
  a20-f45  21    45  20  no    yes    16  1 / 1   159 744 / 162 560  2      1     2      5     1 / 1       near capacity back; the last F on tiles of 16 at A 20
  a20-f46  21    46  20  yes   yes    8   4 / 4   116 480 / 127 744  3      2     2      5     2 / 8       the first F on tiles of 8 at A 20
  a20-f40  21    40  20  no    no     16  2 / 2   153 088 / 158 720  2      1     2      5     1 / 2       two wavefronts each way
  a20-f43  21    43  20  yes   no     16  2 / 1   163 072 / 155 904  2      1     2      5     1 / 1       forward 2 against backward 1
  a20-f36  37    36  20  no    yes    16  4 / 2   159 744 / 145 408  3      2     2      5     2 / 4       forward 4 against backward 2, three tiles
  a24-f38  21    38  24  yes   yes    16  1 / 1   155 904 / 161 024  2      1     2      5     1 / 1       near capacity back; the last F on tiles of 16 at A 24
  a24-f39  21    39  24  no    yes    8   4 / 4   114 816 / 135 296  3      2     2      5     2 / 8       the first F on tiles of 8 at A 24
  a24-f34  37    34  24  no    no     16  2 / 2   150 528 / 160 768  3      2     2      5     2 / 4       two each way on two workgroups
  a28-f33  21    33  28  no    yes    16  2 / 1   163 584 / 161 024  2      1     2      5     1 / 1       near capacity both ways; the last F on 16 at A 28
  a28-f34  21    34  28  yes   yes    8   4 / 4   113 920 / 143 616  3      2     2      5     2 / 8       the first F on tiles of 8 at A 28
  a28-f30  37    30  28  no    yes    16  4 / 1   148 992 / 147 968  3      2     2      5     2 / 2       forward 4 against a lone backward wavefront
  a28-f44  21    44  28  no    no     8   4 / 2   135 680 / 130 560  3      2     2      5     2 / 4       tiles of 8 with two backward wavefronts
  a28-f5   37    5   28  yes   yes    16  4 / 4   38 144 / 91 392    3      2     2      5     2 / 8       a partial second tile with everything else small
  a32-f29  37    29  32  no    yes    16  4 / 1   159 488 / 160 768  3      2     2      5     2 / 2       near capacity back; forward 4 against backward 1
  a16-f44  21    44  16  no    yes    16  4 / 2   163 840 / 144 896  2      1     2      5     1 / 2       the forward at exactly kFgLdsCap, the last F with 4
  a16-f45  21    45  16  yes   no     16  2 / 2   146 688 / 147 712  2      1     2      5     1 / 2       the forward's 2 wavefronts at NE 1
  a16-f48  21    48  16  no    yes    16  2 / 2   155 136 / 156 160  2      1     2      5     1 / 2       the most fields a launch takes
  cap      8200  2   4   no    yes    16  4 / 4   7 680 / 16 896     513    256   3      8     256 / 1024  513 tiles on kFgMaxGrid workgroups, a third trip
B = 21 is two tiles of 16 on one workgroup with 5 samples in the second, or three tiles of 8 on two workgroups (asserted);
B = 37 is three tiles of 16 on two workgroups.  No case has more than 60 000 leaky-relu arguments, so ``w_attn`` stays at unit
scale everywhere (the rule of test_gpu_fignn._case, w_scale 8 above that, is kept in ``make``).  Run-to-run bits at cap and at
a24-f38, a lone wavefront each way.

tests/test_fignn_host.py asserts on the CPU that every case draws a seed, reaches the form of its line, that the ranges the
.hip file's header quotes come out of the restatement, and that the fp32 restatement and the fp32 composition hold the bar
against float64, before anything runs on a GPU.

No figure of this module had been measured on a GPU when it was written.  Measured on the MI355X afterwards, worst err / bar
over the module (22 tests, 4 s; the slowest case 0.5 s): y 0.068, g 0.180, dh 0.267, dh0 0.047, dw_attn 0.168, dW_out 0.212,
dW_in 0.163, dbias_p 0.231, dw_ih 0.350, dw_hh 0.530, db_ih 0.185, db_hh 0.272 -- every kernel holds the bar on every form and
none had to be changed.  Mutation check (a scratch build, never committed; wrong numbers only, in bounds, terminating), failed
here / all passed in the existing module tests/test_gpu_fignn.py (100 tests): fignn_step_bwd_kernel with a lone wavefront
leaving the last field out of its dw_ih / dw_hh accumulation 6 failed here (the six cases with nw_bwd 1: a20-f45, a20-f43,
a24-f38, a28-f33, a28-f30, a32-f29) / all passed in the existing module.  profiles/fignn/INDEX.md quotes the same."""
import functools
import os
import re

import pytest
import torch

import fignn64 as fg
import fp32_bar

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_OPT_IN = 64 * 1024

# name -> (B, F, A, same, want_graph), and what the case has to reach (keys of ``forms``)
CASES = {
    "a20-f45": ((21, 45, 20, False, True),
        {"T": 16, "NE": 2, "nw_fwd": 1, "nw_bwd": 1, "fwd_lds": 159744, "bwd_lds": 162560,
         "tiles": 2, "grid": 1, "trips": 2, "last": 5, "rows1": 1, "rows2": 1}),
    "a20-f46": ((21, 46, 20, True, True),
        {"T": 8, "NE": 2, "nw_fwd": 4, "nw_bwd": 4, "fwd_lds": 116480, "bwd_lds": 127744,
         "tiles": 3, "grid": 2, "trips": 2, "last": 5, "rows1": 2, "rows2": 8}),
    "a20-f40": ((21, 40, 20, False, False),
        {"T": 16, "NE": 2, "nw_fwd": 2, "nw_bwd": 2, "fwd_lds": 153088, "bwd_lds": 158720,
         "tiles": 2, "grid": 1, "trips": 2, "last": 5, "rows1": 1, "rows2": 2}),
    "a20-f43": ((21, 43, 20, True, False),
        {"T": 16, "NE": 2, "nw_fwd": 2, "nw_bwd": 1, "fwd_lds": 163072, "bwd_lds": 155904,
         "tiles": 2, "grid": 1, "trips": 2, "last": 5, "rows1": 1, "rows2": 1}),
    "a20-f36": ((37, 36, 20, False, True),
        {"T": 16, "NE": 2, "nw_fwd": 4, "nw_bwd": 2, "fwd_lds": 159744, "bwd_lds": 145408,
         "tiles": 3, "grid": 2, "trips": 2, "last": 5, "rows1": 2, "rows2": 4}),
    "a24-f38": ((21, 38, 24, True, True),
        {"T": 16, "NE": 2, "nw_fwd": 1, "nw_bwd": 1, "fwd_lds": 155904, "bwd_lds": 161024,
         "tiles": 2, "grid": 1, "trips": 2, "last": 5, "rows1": 1, "rows2": 1}),
    "a24-f39": ((21, 39, 24, False, True),
        {"T": 8, "NE": 2, "nw_fwd": 4, "nw_bwd": 4, "fwd_lds": 114816, "bwd_lds": 135296,
         "tiles": 3, "grid": 2, "trips": 2, "last": 5, "rows1": 2, "rows2": 8}),
    "a24-f34": ((37, 34, 24, False, False),
        {"T": 16, "NE": 2, "nw_fwd": 2, "nw_bwd": 2, "fwd_lds": 150528, "bwd_lds": 160768,
         "tiles": 3, "grid": 2, "trips": 2, "last": 5, "rows1": 2, "rows2": 4}),
    "a28-f33": ((21, 33, 28, False, True),
        {"T": 16, "NE": 2, "nw_fwd": 2, "nw_bwd": 1, "fwd_lds": 163584, "bwd_lds": 161024,
         "tiles": 2, "grid": 1, "trips": 2, "last": 5, "rows1": 1, "rows2": 1}),
    "a28-f34": ((21, 34, 28, True, True),
        {"T": 8, "NE": 2, "nw_fwd": 4, "nw_bwd": 4, "fwd_lds": 113920, "bwd_lds": 143616,
         "tiles": 3, "grid": 2, "trips": 2, "last": 5, "rows1": 2, "rows2": 8}),
    "a28-f30": ((37, 30, 28, False, True),
        {"T": 16, "NE": 2, "nw_fwd": 4, "nw_bwd": 1, "fwd_lds": 148992, "bwd_lds": 147968,
         "tiles": 3, "grid": 2, "trips": 2, "last": 5, "rows1": 2, "rows2": 2}),
    "a28-f44": ((21, 44, 28, False, False),
        {"T": 8, "NE": 2, "nw_fwd": 4, "nw_bwd": 2, "fwd_lds": 135680, "bwd_lds": 130560,
         "tiles": 3, "grid": 2, "trips": 2, "last": 5, "rows1": 2, "rows2": 4}),
    "a28-f5": ((37, 5, 28, True, True),
        {"T": 16, "NE": 2, "nw_fwd": 4, "nw_bwd": 4, "fwd_lds": 38144, "bwd_lds": 91392,
         "tiles": 3, "grid": 2, "trips": 2, "last": 5, "rows1": 2, "rows2": 8}),
    "a32-f29": ((37, 29, 32, False, True),
        {"T": 16, "NE": 2, "nw_fwd": 4, "nw_bwd": 1, "fwd_lds": 159488, "bwd_lds": 160768,
         "tiles": 3, "grid": 2, "trips": 2, "last": 5, "rows1": 2, "rows2": 2}),
    "a16-f44": ((21, 44, 16, False, True),
        {"T": 16, "NE": 1, "nw_fwd": 4, "nw_bwd": 2, "fwd_lds": 163840, "bwd_lds": 144896,
         "tiles": 2, "grid": 1, "trips": 2, "last": 5, "rows1": 1, "rows2": 2}),
    "a16-f45": ((21, 45, 16, True, False),
        {"T": 16, "NE": 1, "nw_fwd": 2, "nw_bwd": 2, "fwd_lds": 146688, "bwd_lds": 147712,
         "tiles": 2, "grid": 1, "trips": 2, "last": 5, "rows1": 1, "rows2": 2}),
    "a16-f48": ((21, 48, 16, False, True),
        {"T": 16, "NE": 1, "nw_fwd": 2, "nw_bwd": 2, "fwd_lds": 155136, "bwd_lds": 156160,
         "tiles": 2, "grid": 1, "trips": 2, "last": 5, "rows1": 1, "rows2": 2}),
    "cap": ((8200, 2, 4, False, True),
        {"T": 16, "NE": 1, "nw_fwd": 4, "nw_bwd": 4, "fwd_lds": 7680, "bwd_lds": 16896,
         "tiles": 513, "grid": 256, "trips": 3, "last": 8, "rows1": 256, "rows2": 1024}),
}
# (F, A) -> LDS bytes of the shapes closest to the capacity, forward and backward
NEAR_CAP_FWD = {(33, 28): 163584, (44, 16): 163840}
NEAR_CAP_BWD = {(45, 20): 162560, (38, 24): 161024, (33, 28): 161024, (29, 32): 160768}
SWITCH = {20: (45, 46), 24: (38, 39), 28: (33, 34)}                    # A -> the last F on tiles of 16, the first on tiles of 8
# (T, nw_fwd, nw_bwd): every combination the host side can select over the supported range
COMBOS = {(16, 4, 4), (16, 4, 2), (16, 2, 2), (16, 2, 1), (16, 1, 1), (16, 4, 1), (8, 4, 4), (8, 4, 2)}
BITS = ("cap", "a24-f38")


# ---- the launch geometry, restated ---------------------------------------------------------------------------------------------
def _ceil(a, b):
    return -(-a // b)


def _pad16(n):
    return (n + 15) & ~15


@functools.lru_cache(maxsize=None)
def constants():
    """The constants of csrc/rbx_fignn.hip the restatement depends on, read from the source; the lines of the LDS layout, of the
    tile and wavefront choice and of the grid are held to their text."""
    with open(os.path.join(ROOT, "recbox_amd", "csrc", "rbx_fignn.hip")) as fh:
        text = fh.read()
    k = {name: int(re.search(r"\b%s = (\d+)" % name, text).group(1)) for name in ("kFgMinF", "kFgMaxF", "kFgMinA", "kFgMaxA",
                                                                                  "kFgTile", "kFgMaxGrid")}
    a, b = re.search(r"\bkFgLdsCap = (\d+) \* (\d+);", text).groups()
    k["kFgLdsCap"] = int(a) * int(b)
    assert "const int FP = fg_pad16(F), plane = FP * (FP + 4);" in text
    assert "const int field = bwd ? kFgTile * (3 * (A + 4) + 2 * (3 * A + 4)) : kFgTile * 2 * (A + 4);" in text
    assert "return plane > field ? plane : field;" in text
    assert "{ return 2 * F * T * (A + 4) + 4 * F * T; }" in text
    assert "return 4 * (static_cast<size_t>(fg_shared(F, A, T)) + static_cast<size_t>(nw) * fg_scratch(F, A, bwd));" in text
    assert "{ return fg_lds(F, A, true, 1, kFgTile) <= kFgLdsCap ? kFgTile : kFgTile / 2; }" in text
    assert "for (int nw = 4; nw > 1; nw >>= 1)" in text and "if (fg_lds(F, A, bwd, nw, T) <= kFgLdsCap) return nw;" in text
    assert "const int64_t tiles = (batch + T - 1) / T, need = (tiles + 1) / 2;" in text
    assert "return static_cast<unsigned>(need < kFgMaxGrid ? need : kFgMaxGrid);" in text
    assert "{ return 2 * F * A * A; }" in text and "{ return 6 * A * A + 9 * A; }" in text
    assert "return (grid * fg_row1(n_fields, dim) + grid * nw * fg_row2(dim)) * sizeof(float);" in text
    assert "t.rows1 = static_cast<int>(grid); t.rows2 = static_cast<int>(grid) * nw;" in text
    assert "const int lrc = dim <= 16 ?" in text
    return k


def lds(F, A, bwd, nw, T, k=None):
    """``fg_lds``: the bytes of X, Y, s, d, ds, dd and of nw wavefronts' scratch."""
    k = k or constants()
    FP = _pad16(F)
    field = k["kFgTile"] * (3 * (A + 4) + 2 * (3 * A + 4)) if bwd else k["kFgTile"] * 2 * (A + 4)
    return 4 * (2 * F * T * (A + 4) + 4 * F * T + nw * max(FP * (FP + 4), field))


def tile(F, A, k=None):
    """``fg_tile``: 16 samples where one backward wavefront's LDS holds that, else 8."""
    k = k or constants()
    return k["kFgTile"] if lds(F, A, True, 1, k["kFgTile"], k) <= k["kFgLdsCap"] else k["kFgTile"] // 2


def waves(F, A, bwd, k=None):
    k = k or constants()
    return next((n for n in (4, 2) if lds(F, A, bwd, n, tile(F, A, k), k) <= k["kFgLdsCap"]), 1)


def forms(B, F, A, k=None):
    """Every host-side quantity of the forward and backward launches for one shape (see the module's docstring)."""
    k = k or constants()
    T = tile(F, A, k)
    q = {"T": T, "NE": 1 if A <= 16 else 2, "nw_fwd": waves(F, A, False, k), "nw_bwd": waves(F, A, True, k)}
    q["fwd_lds"], q["bwd_lds"] = lds(F, A, False, q["nw_fwd"], T, k), lds(F, A, True, q["nw_bwd"], T, k)
    q["tiles"] = _ceil(B, T)
    q["grid"] = min((q["tiles"] + 1) // 2, k["kFgMaxGrid"])
    q["trips"] = _ceil(q["tiles"], q["grid"])
    q["last"] = B - (q["tiles"] - 1) * T
    q["rows1"], q["rows2"] = q["grid"], q["grid"] * q["nw_bwd"]
    return q


def supported(F, A, k=None):
    k = k or constants()
    return (k["kFgMinF"] <= F <= k["kFgMaxF"] and k["kFgMinA"] <= A <= k["kFgMaxA"] and A % 4 == 0
            and lds(F, A, True, 1, tile(F, A, k), k) <= k["kFgLdsCap"])


def check_forms(name):
    """The case reaches what the table says it reaches; the workspace rows agree with the library's."""
    from recbox_amd import _lib
    (B, F, A, _, _), expect = CASES[name]
    k = constants()
    q = forms(B, F, A, k)
    for key, value in expect.items():
        assert q[key] == value, "%s: %s is %d, the table says %d" % (name, key, q[key], value)
    assert supported(F, A, k) and _lib.lib.rbx_fignn_step_supported(F, A) == 1, name
    assert _lib.lib.rbx_fignn_step_bwd_workspace_size(B, F, A) == 4 * (q["rows1"] * 2 * F * A * A + q["rows2"] * (6 * A * A + 9 * A)), name
    assert max(q["fwd_lds"], q["bwd_lds"]) <= k["kFgLdsCap"]
    if B == 21:                                                        # two tiles of 16 on one workgroup, or three of 8 on two
        assert (q["tiles"], q["grid"], q["trips"], q["last"]) == ((2, 1, 2, 5) if q["T"] == 16 else (3, 2, 2, 5)), name
    return q


def check_the_list_covers_every_form():
    """Over the whole list: what the module's docstring promises, so that a case taken out of ``CASES`` fails here."""
    k = constants()
    assert (k["kFgTile"], k["kFgMaxF"], k["kFgMaxA"], k["kFgMaxGrid"], k["kFgLdsCap"]) == (16, 48, 32, 256, 163840)
    shapes = {name: c[0] for name, c in CASES.items()}
    qs = {name: forms(*s[:3], k=k) for name, s in shapes.items()}
    combo = {n: (q["T"], q["nw_fwd"], q["nw_bwd"]) for n, q in qs.items()}
    assert set(combo.values()) >= COMBOS
    for A in (20, 24, 28):                                             # every partial width on both tile sizes and with one wavefront
        mine = [n for n, s in shapes.items() if s[2] == A]
        assert {qs[n]["T"] for n in mine} == {16, 8} and all(qs[n]["NE"] == 2 for n in mine), A
        assert any(qs[n]["nw_bwd"] == 1 for n in mine), A
        last16, first8 = SWITCH[A]
        assert any(shapes[n][1] == last16 and qs[n]["T"] == 16 for n in mine), A
        assert any(shapes[n][1] == first8 and qs[n]["T"] == 8 for n in mine), A
    widths = {c: {s[2] for n, s in shapes.items() if combo[n] == c} for c in COMBOS}           # each combination at these widths
    assert widths[(16, 1, 1)] >= {20, 24} and widths[(16, 2, 2)] >= {16, 20, 24} and widths[(16, 2, 1)] >= {20, 28}
    assert widths[(16, 4, 2)] >= {16, 20} and widths[(16, 4, 1)] >= {28, 32} and widths[(8, 4, 4)] >= {20, 24, 28}
    assert widths[(8, 4, 2)] >= {28} and widths[(16, 4, 4)] >= {4, 28}
    at16 = {s[1]: qs[n]["nw_fwd"] for n, s in shapes.items() if s[2] == 16}                     # the forward's 4 -> 2 at NE = 1
    assert at16 == {44: 4, 45: 2, 48: 2}
    assert any(s[:3] == (21, 48, 16) for s in shapes.values())                                 # the most fields a launch takes
    assert any(s[2] == 28 and s[1] < 16 and combo[n] == (16, 4, 4) for n, s in shapes.items())  # a partial tile, everything small
    for (F, A), b in NEAR_CAP_FWD.items():
        assert any(s[1:3] == (F, A) and qs[n]["fwd_lds"] == b for n, s in shapes.items()), (F, A)
    for (F, A), b in NEAR_CAP_BWD.items():
        assert any(s[1:3] == (F, A) and qs[n]["bwd_lds"] == b for n, s in shapes.items()), (F, A)
    assert combo["a32-f29"] == (16, 4, 1)
    assert min(q["fwd_lds"] for q in qs.values() if q["NE"] == 2) < LDS_OPT_IN < max(q["fwd_lds"] for q in qs.values())
    assert min(q["bwd_lds"] for q in qs.values()) < LDS_OPT_IN < max(q["bwd_lds"] for q in qs.values())
    cap = qs["cap"]
    assert (cap["tiles"], cap["grid"], cap["trips"], cap["last"], cap["rows1"], cap["rows2"]) == (513, 256, 3, 8, 256, 1024)
    assert any(s[0] == 37 and q["T"] == 16 and (q["tiles"], q["grid"], q["trips"]) == (3, 2, 2) for s, q in
               ((shapes[n], qs[n]) for n in qs))
    for A in (20, 24, 28):
        assert {s[3] for s in shapes.values() if s[2] == A} == {True, False}, A
        assert {s[4] for s in shapes.values() if s[2] == A} == {True, False}, A
    assert {(s[3], s[4]) for s in shapes.values()} == {(a, b) for a in (True, False) for b in (True, False)}
    assert qs[BITS[0]]["trips"] == 3 and combo[BITS[1]] == (16, 1, 1)


def header_figures():
    """The (F, A) ranges the file's header and the issue quote, from the restatement: {A: first F on tiles of 8}, and for every
    supported shape its (T, nw_fwd, nw_bwd)."""
    k = constants()
    first8 = {A: min(F for F in range(2, 49) if supported(F, A, k) and tile(F, A, k) == 8) for A in (20, 24, 28, 32)}
    combos = {(F, A): (tile(F, A, k), waves(F, A, False, k), waves(F, A, True, k))
              for A in range(4, 33, 4) for F in range(2, 49) if supported(F, A, k)}
    return first8, combos


@functools.lru_cache(maxsize=None)
def make(name):
    """The rule of test_gpu_fignn._case: above 60 000 leaky-relu arguments w_attn is drawn 8 times wider (no case here is)."""
    B, F, A, same, _ = CASES[name][0]
    return fg.make_case(B, F, A, 0, same, 8.0 if B * F * F > 60000 else 1.0)


@functools.lru_cache(maxsize=None)
def refs(name):
    """(float64, fp32 on the CPU) of a case, computed once."""
    return fg.reference(make(name)), fg.ref32(make(name))


# ---- the tests -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(autouse=True)
def fused_only(monkeypatch):
    """The kernels over their whole range, whatever the default routing; the composition fails the test; the calls that reach
    rbx_fignn_step_fwd are counted."""
    from recbox_amd import ops
    monkeypatch.setattr(ops.config, "fignn_fused", True)
    monkeypatch.setattr(ops.config, "fignn_fields", ops.FIGNN_MAX_FIELDS)
    monkeypatch.setattr(ops.config, "fignn_dim", ops.FIGNN_MAX_DIM)
    monkeypatch.setattr(ops, "fignn_step_torch", lambda *a, **k: pytest.fail("the fused step did not run"))
    calls = []
    fwd = ops.lib.rbx_fignn_step_fwd
    monkeypatch.setattr(ops.lib, "rbx_fignn_step_fwd", lambda *a: (calls.append(1), fwd(*a))[1])
    return calls


def _fused(*a):
    from recbox_amd import ops
    return ops.fignn_step(*a)


def _run(name):
    return fg.run(_fused, make(name), "cuda", want_graph=CASES[name][0][4])


def test_the_list_covers_every_form():
    check_the_list_covers_every_form()


@pytest.mark.parametrize("name", list(CASES))
def test_form_matches_float64_under_the_fp32_bar(name, fused_only):
    q = check_forms(name)
    print("%s: %s" % (name, ", ".join("%s %d" % kv for kv in sorted(q.items()))))
    want, ref32 = refs(name)
    got = _run(name)
    assert len(fused_only) == 1
    assert CASES[name][0][4] or got["g"] is None
    for n in fg.NAMES:
        if want[n] is None or (n == "g" and not CASES[name][0][4]):
            assert got[n] is None, n
        else:
            fp32_bar.assert_bar("%s %s" % (n, name), got[n], want[n], ref32[n])


@pytest.mark.parametrize("name", BITS)
def test_two_runs_give_the_same_bits(name, fused_only):
    q = check_forms(name)
    assert q["trips"] == 3 or (q["nw_fwd"], q["nw_bwd"]) == (1, 1)
    first, second = _run(name), _run(name)
    assert len(fused_only) == 2
    for n in fg.NAMES:
        if first[n] is None or second[n] is None:
            assert first[n] is None and second[n] is None, n
        else:
            assert torch.equal(first[n], second[n]), (name, n)


def test_report_worst_ratio():
    """Prints the worst err / bar per tensor over this module."""
    fp32_bar.report("fignn forms")
