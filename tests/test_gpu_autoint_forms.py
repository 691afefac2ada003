"""AutoInt's field self-attention layer (``ops.field_attn``, csrc/rbx_fieldattn.hip) at every width and launch form its host side
can select, against the float64 restatement of tests/fieldattn64.py under the bar of tests/fp32_bar.py: per tensor
max|got - want| <= max(4 e32, 2e-6 max|want|), e32 the error of the fp32 composition on the CPU.  Every name of
``fieldattn64.NAMES`` and ``attn`` is held to it in every case; the composition is patched to fail and the C forward entry is
counted, so a fall-back cannot pass.  tests/test_gpu_autoint.py runs E in {4, 8, 12, 16, 32} only, backward wavefront counts of
4, 2 and 1 only and at most 600 workspace rows; the forms below lie beyond it.

The host-side quantities, restated here from the .hip file (``forms``; FP = F rounded up to 16):
  w        = (pad16(3 E) + pad16(E)) (E + 4) floats of staged weights (pad16(3 E) != 3 E at E = 20 and 28)
  wave     = FP (2 (E + 4) + (3 E + 4) + (FP + 4)) floats forward, FP (4 (E + 4) + 2 (3 E + 4) + 2 (FP + 4)) backward
  nw       = the largest of 4, 3, 2 with 4 (w + nw wave) <= kFaLdsCap, else 1; LDS = 4 (w + nw wave), opted in above 64 KiB
  grid     = min(ceil(B / (2 nw)), kFaMaxGrid); trips = ceil(B / (grid nw)) of wavefront 0; rows = grid nw of the backward, the
             workspace's rows (read from the library too: they must agree); chunks = ceil(rows / 16) of the tail
  NE       = 1 up to E = 16, else 2: the backward's accumulator tiles per side; at E = 20, 24, 28 the second one is partial

  case     B     F   E   h  res  relu  bias  FP  nw f/b  LDS fwd / bwd      grid f/b   rows  trips  what it is here for
  e20-f5   37    5   20  5  yes  yes   yes   16  4 / 4   43 008 / 76 800    5 / 5      20    2 / 2  dh 4 at E 20; the forward below 64 KiB
  e20-f32  37    32  20  1  yes  yes   yes   32  4 / 4   84 992 / 160 768   5 / 5      20    2 / 2  dh 20; near capacity at nw 4
  e20-f48  37    48  20  5  yes  yes   yes   48  4 / 2   135 168 / 135 168  5 / 10     20    2 / 2  FP 48 at E 20: two wavefronts back
  e24-f20  37    20  24  6  yes  yes   yes   32  4 / 3   98 560 / 141 568   5 / 7      21    2 / 2  nw 3 at a partial second tile, h 6
  e24-f18  37    18  24  3  yes  yes   yes   32  4 / 3   98 560 / 141 568   5 / 7      21    2 / 2  the same form at h 3 (dh 8); a dropout shape
  e24-f48  37    48  24  2  no   no    yes   48  4 / 2   153 856 / 153 856  5 / 10     20    2 / 2  dh 12 at FP 48; no epilogue at all
  e28-f7   37    7   28  7  no   yes   no    16  4 / 4   60 416 / 104 448   5 / 5      20    2 / 2  dh 4 at E 28; relu alone, no bias
  e28-f32  37    32  28  7  yes  yes   yes   32  4 / 3   112 640 / 160 768  5 / 7      21    2 / 2  near capacity at nw 3, F = FP
  e28-f48  37    48  28  1  yes  yes   yes   48  3 / 1   133 888 / 94 720   7 / 19     19    2 / 2  dh 28; forward nw 3, backward nw 1
  e12-f40  37    40  12  3  yes  yes   yes   48  4 / 3   99 328 / 146 944   5 / 7      21    2 / 2  nw 3 at NE 1, F < FP; a dropout shape
  e12-f48  37    48  12  3  yes  yes   yes   48  4 / 3   99 328 / 146 944   5 / 7      21    2 / 2  nw 3 at NE 1, F = FP
  e8-f48   37    48  8   2  yes  yes   yes   48  4 / 4   82 176 / 162 048   5 / 5      20    2 / 2  near capacity at nw 4, NE 1
  cap-nw4  4099  2   4   1  yes  yes   yes   16  4 / 4   14 336 / 27 648    512 / 512  2048  3 / 3  both grid caps, third trips, 128 chunks
  cap-nw1  1027  48  32  8  yes  no    no    48  3 / 1   147 456 / 104 448  172 / 512  512   2 / 3  the backward's cap at nw 1, 32 chunks
B = 37 gives rows < B < 2 rows at every nw: every wavefront takes a second trip and the last workgroups' is partial or empty
(asserted).  cap-nw1 carries 1.6 M pre-activations, no seed of ``fieldattn64.make_case`` keeps them all 1e-5 from zero, so it
runs without relu; its third trip holds 3 samples on 512 workgroups.  Dropout (p = 0.25, a fixed seed, the kernels' own mask
from ``ops.attention_dropout_mask``) runs at (37, 18, 24, 3), (37, 40, 12, 3) and (37, 48, 32, 8): a partial second tile,
backward nw 3, and nw 1 at FP 48 with E > 16.  Run-to-run bits at the two cap cases and at e24-f20.

tests/test_autoint_host.py asserts on the CPU that every case draws a seed, reaches the form of its line, and that the fp32
composition holds the bar against float64, before anything runs on a GPU.

No figure of this module had been measured on a GPU when it was written.  Measured on the MI355X afterwards, worst err / bar
over the module (22 tests, 3 s; the slowest, cap-nw1, 0.6 s): attn 0.250, dWin 0.174, dWout 0.154, dbin 0.184, dbout 0.113,
dres 0.000, dx 0.257, y 0.135 -- every kernel holds the bar on every form and none had to be changed.  Mutation check (a
scratch build, never committed; wrong numbers only, in bounds, terminating), failed here / all passed in the existing module
tests/test_gpu_autoint.py (100 tests): fieldattn_bwd_kernel writing column c of a partial second tile's dWin from the first
tile's accumulator 10 failed here (the nine cases at E 20, 24, 28 and the dropout case at E 24) / all passed in the existing
module; the same kernel staging the second trip's x again on a third trip 2 failed here (cap-nw4, cap-nw1) / all passed in the
existing module.  profiles/autoint/INDEX.md quotes the same."""
import functools
import os
import re

import pytest
import torch

import fieldattn64 as fa
import fp32_bar

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_OPT_IN = 64 * 1024
ALL = fa.NAMES + ("attn",)
FORMS = [(False, False, True), (True, True, True), (True, False, False), (False, True, False)]     # test_gpu_autoint.FORMS

# name -> (B, F, E, h, residual, relu, biases), and what the case has to reach (keys of ``forms``)
CASES = {
    "e20-f5": ((37, 5, 20, 5, True, True, True),
        {"FP": 16, "NE": 2, "nw_fwd": 4, "nw_bwd": 4, "fwd_lds": 43008, "bwd_lds": 76800,
         "grid_fwd": 5, "grid_bwd": 5, "rows": 20, "trips_fwd": 2, "trips_bwd": 2, "chunks": 2}),
    "e20-f32": ((37, 32, 20, 1, True, True, True),
        {"FP": 32, "NE": 2, "nw_fwd": 4, "nw_bwd": 4, "fwd_lds": 84992, "bwd_lds": 160768,
         "grid_fwd": 5, "grid_bwd": 5, "rows": 20, "trips_fwd": 2, "trips_bwd": 2, "chunks": 2}),
    "e20-f48": ((37, 48, 20, 5, True, True, True),
        {"FP": 48, "NE": 2, "nw_fwd": 4, "nw_bwd": 2, "fwd_lds": 135168, "bwd_lds": 135168,
         "grid_fwd": 5, "grid_bwd": 10, "rows": 20, "trips_fwd": 2, "trips_bwd": 2, "chunks": 2}),
    "e24-f20": ((37, 20, 24, 6, True, True, True),
        {"FP": 32, "NE": 2, "nw_fwd": 4, "nw_bwd": 3, "fwd_lds": 98560, "bwd_lds": 141568,
         "grid_fwd": 5, "grid_bwd": 7, "rows": 21, "trips_fwd": 2, "trips_bwd": 2, "chunks": 2}),
    "e24-f18": ((37, 18, 24, 3, True, True, True),
        {"FP": 32, "NE": 2, "nw_fwd": 4, "nw_bwd": 3, "fwd_lds": 98560, "bwd_lds": 141568,
         "grid_fwd": 5, "grid_bwd": 7, "rows": 21, "trips_fwd": 2, "trips_bwd": 2, "chunks": 2}),
    "e24-f48": ((37, 48, 24, 2, False, False, True),
        {"FP": 48, "NE": 2, "nw_fwd": 4, "nw_bwd": 2, "fwd_lds": 153856, "bwd_lds": 153856,
         "grid_fwd": 5, "grid_bwd": 10, "rows": 20, "trips_fwd": 2, "trips_bwd": 2, "chunks": 2}),
    "e28-f7": ((37, 7, 28, 7, False, True, False),
        {"FP": 16, "NE": 2, "nw_fwd": 4, "nw_bwd": 4, "fwd_lds": 60416, "bwd_lds": 104448,
         "grid_fwd": 5, "grid_bwd": 5, "rows": 20, "trips_fwd": 2, "trips_bwd": 2, "chunks": 2}),
    "e28-f32": ((37, 32, 28, 7, True, True, True),
        {"FP": 32, "NE": 2, "nw_fwd": 4, "nw_bwd": 3, "fwd_lds": 112640, "bwd_lds": 160768,
         "grid_fwd": 5, "grid_bwd": 7, "rows": 21, "trips_fwd": 2, "trips_bwd": 2, "chunks": 2}),
    "e28-f48": ((37, 48, 28, 1, True, True, True),
        {"FP": 48, "NE": 2, "nw_fwd": 3, "nw_bwd": 1, "fwd_lds": 133888, "bwd_lds": 94720,
         "grid_fwd": 7, "grid_bwd": 19, "rows": 19, "trips_fwd": 2, "trips_bwd": 2, "chunks": 2}),
    "e12-f40": ((37, 40, 12, 3, True, True, True),
        {"FP": 48, "NE": 1, "nw_fwd": 4, "nw_bwd": 3, "fwd_lds": 99328, "bwd_lds": 146944,
         "grid_fwd": 5, "grid_bwd": 7, "rows": 21, "trips_fwd": 2, "trips_bwd": 2, "chunks": 2}),
    "e12-f48": ((37, 48, 12, 3, True, True, True),
        {"FP": 48, "NE": 1, "nw_fwd": 4, "nw_bwd": 3, "fwd_lds": 99328, "bwd_lds": 146944,
         "grid_fwd": 5, "grid_bwd": 7, "rows": 21, "trips_fwd": 2, "trips_bwd": 2, "chunks": 2}),
    "e8-f48": ((37, 48, 8, 2, True, True, True),
        {"FP": 48, "NE": 1, "nw_fwd": 4, "nw_bwd": 4, "fwd_lds": 82176, "bwd_lds": 162048,
         "grid_fwd": 5, "grid_bwd": 5, "rows": 20, "trips_fwd": 2, "trips_bwd": 2, "chunks": 2}),
    "cap-nw4": ((4099, 2, 4, 1, True, True, True),
        {"FP": 16, "NE": 1, "nw_fwd": 4, "nw_bwd": 4, "fwd_lds": 14336, "bwd_lds": 27648,
         "grid_fwd": 512, "grid_bwd": 512, "rows": 2048, "trips_fwd": 3, "trips_bwd": 3, "chunks": 128}),
    "cap-nw1": ((1027, 48, 32, 8, True, False, False),
        {"FP": 48, "NE": 2, "nw_fwd": 3, "nw_bwd": 1, "fwd_lds": 147456, "bwd_lds": 104448,
         "grid_fwd": 172, "grid_bwd": 512, "rows": 512, "trips_fwd": 2, "trips_bwd": 3, "chunks": 32}),
}
NEAR_CAP = {(48, 8): 162048, (32, 20): 160768, (32, 28): 160768}          # (FP, E) -> the backward's LDS bytes
DROP = [(37, 18, 24, 3), (37, 40, 12, 3), (37, 48, 32, 8)]
BITS = ("cap-nw4", "cap-nw1", "e24-f20")


# ---- the launch geometry, restated ---------------------------------------------------------------------------------------------
def _ceil(a, b):
    return -(-a // b)


def _pad16(n):
    return (n + 15) & ~15


@functools.lru_cache(maxsize=None)
def constants():
    """The constants of csrc/rbx_fieldattn.hip the restatement depends on, read from the source; the lines of the layout, of the
    wavefront count and of the grid are held to their text."""
    with open(os.path.join(ROOT, "recbox_amd", "csrc", "rbx_fieldattn.hip")) as fh:
        text = fh.read()
    k = {name: int(re.search(r"\b%s = (\d+)" % name, text).group(1)) for name in ("kFaMinF", "kFaMaxF", "kFaMinE", "kFaMaxE",
                                                                                  "kFaMaxH", "kFaMaxGrid")}
    a, b = re.search(r"\bkFaLdsCap = (\d+) \* (\d+);", text).groups()
    k["kFaLdsCap"] = int(a) * int(b)
    assert "return (fa_pad16(3 * E) + fa_pad16(E)) * (E + 4); }" in text and "return 4 * E * E + 4 * E; }" in text
    assert "return FP * (2 * (E + 4) + (3 * E + 4) + (FP + 4));" in text
    assert "return FP * (4 * (E + 4) + 2 * (3 * E + 4) + 2 * (FP + 4));" in text
    assert "for (int nw = 4; nw > 1; --nw)" in text
    assert "if (4 * (fa_w_floats(E) + static_cast<size_t>(nw) * wave_floats) <= kFaLdsCap) return nw;" in text
    assert "const int64_t need = (batch + 2 * nw - 1) / (2 * nw);" in text
    assert "return static_cast<unsigned>(need < kFaMaxGrid ? need : kFaMaxGrid);" in text
    assert "if (lds > 64 * 1024) (void)hipFuncSetAttribute(" in text and "if (dim <= 16) {" in text
    assert "static_cast<int>(grid) * nw, dim, d_din_w, d_din_b, d_dout_w, d_dout_b);" in text
    return k


def waves(E, wave_floats, k=None):
    """(nw, LDS bytes) of ``fa_waves`` for one direction."""
    k = k or constants()
    w = (_pad16(3 * E) + _pad16(E)) * (E + 4)
    nw = next((n for n in (4, 3, 2) if 4 * (w + n * wave_floats) <= k["kFaLdsCap"]), 1)
    return nw, 4 * (w + nw * wave_floats)


def forms(B, F, E, k=None):
    """Every host-side quantity of the forward and backward launches for one shape (see the module's docstring)."""
    k = k or constants()
    FP = _pad16(F)
    q = {"FP": FP, "NE": 1 if E <= 16 else 2, "w_floats": (_pad16(3 * E) + _pad16(E)) * (E + 4), "row_len": 4 * E * E + 4 * E}
    q["fwd_wave"] = FP * (2 * (E + 4) + (3 * E + 4) + (FP + 4))
    q["bwd_wave"] = FP * (4 * (E + 4) + 2 * (3 * E + 4) + 2 * (FP + 4))
    for d in ("fwd", "bwd"):
        nw, lds = waves(E, q[d + "_wave"], k)
        q["nw_" + d], q[d + "_lds"] = nw, lds
        q["grid_" + d] = min(_ceil(B, 2 * nw), k["kFaMaxGrid"])
        q["trips_" + d] = _ceil(B, q["grid_" + d] * nw)
    q["rows"] = q["grid_bwd"] * q["nw_bwd"]
    q["chunks"] = _ceil(q["rows"], 16)
    return q


def check_forms(name):
    """The case reaches what the table says it reaches; the workspace rows agree with the library's."""
    from recbox_amd import _lib
    (B, F, E, h, _, _, _), expect = CASES[name]
    k = constants()
    q = forms(B, F, E, k)
    for key, value in expect.items():
        assert q[key] == value, "%s: %s is %d, the table says %d" % (name, key, q[key], value)
    assert _lib.lib.rbx_fieldattn_supported(F, E, h) == 1, name
    assert _lib.lib.rbx_fieldattn_bwd_workspace_size(B, F, E, h) == 4 * q["rows"] * q["row_len"], name
    assert max(q["fwd_lds"], q["bwd_lds"]) <= k["kFaLdsCap"]
    if B == 37:                                                        # every wavefront a second trip, the last ones partial
        assert q["rows"] < B < 2 * q["rows"] and q["grid_fwd"] * q["nw_fwd"] < B < 2 * q["grid_fwd"] * q["nw_fwd"], name
    return q


def check_the_list_covers_every_form():
    """Over the whole list: what the module's docstring promises, so that a case taken out of ``CASES`` fails here."""
    k = constants()
    assert (k["kFaMaxF"], k["kFaMaxE"], k["kFaMaxGrid"], k["kFaLdsCap"]) == (48, 32, 512, 163840)
    shapes = {name: c[0] for name, c in CASES.items()}
    qs = {name: forms(*s[:3], k=k) for name, s in shapes.items()}
    heads = {E: {s[3] for s in shapes.values() if s[2] == E} for E in (20, 24, 28)}
    assert heads[20] >= {1, 5} and heads[24] >= {6, 3, 2} and heads[28] >= {7, 1}
    assert {s[2] // s[3] for s in shapes.values()} >= {4, 8, 12, 20, 28}                      # head widths
    fps = {E: {qs[n]["FP"] for n, s in shapes.items() if s[2] == E} for E in (20, 24, 28)}
    assert fps[20] == fps[28] == {16, 32, 48} and fps[24] == {32, 48}   # FP 32 twice at E 24: two head counts on nw 3
    assert all(q["NE"] == (2 if shapes[n][2] > 16 else 1) for n, q in qs.items())
    for FP in (16, 32, 48):
        assert any(qs[n]["FP"] == FP and s[1] % 16 != 0 for n, s in shapes.items()), FP
    assert {q["nw_bwd"] for q in qs.values()} == {1, 2, 3, 4} and {q["nw_fwd"] for q in qs.values()} >= {3, 4}
    nw3 = [n for n in qs if qs[n]["nw_bwd"] == 3]
    assert {(qs[n]["NE"], shapes[n][1] % 16 == 0) for n in nw3} >= {(1, True), (1, False), (2, True), (2, False)}
    assert {(qs[n]["FP"], shapes[n][2]) for n in nw3} == {(48, 12), (32, 24), (32, 28)}
    assert qs["e24-f20"]["nw_bwd"] == qs["e24-f18"]["nw_bwd"] == 3 and shapes["e24-f20"][3] != shapes["e24-f18"][3]
    assert {(q["FP"], shapes[n][2]) for n, q in qs.items() if q["nw_bwd"] == 2} >= {(48, 20), (48, 24)}
    assert min(q["fwd_lds"] for q in qs.values() if q["NE"] == 2) < LDS_OPT_IN < max(q["fwd_lds"] for q in qs.values())
    assert min(q["bwd_lds"] for q in qs.values()) < LDS_OPT_IN < max(q["bwd_lds"] for q in qs.values())
    for (FP, E), lds in NEAR_CAP.items():
        assert any(q["FP"] == FP and shapes[n][2] == E and q["bwd_lds"] == lds for n, q in qs.items()), (FP, E)
    top = qs["cap-nw4"]
    assert (top["nw_fwd"], top["nw_bwd"], top["grid_fwd"], top["grid_bwd"], top["trips_fwd"], top["trips_bwd"]) == (4, 4, 512, 512, 3, 3)
    assert top["rows"] == k["kFaMaxGrid"] * 4 == 2048
    one = qs["cap-nw1"]
    assert (one["nw_bwd"], one["grid_bwd"], one["trips_bwd"], one["rows"]) == (1, 512, 3, 512) and one["FP"] == 48 and one["NE"] == 2
    assert {s[4:] for s in shapes.values()} == set(FORMS)
    drop = [forms(37, F, E, k) for _, F, E, _ in DROP]
    assert DROP[0][2] % 16 != 0 and drop[0]["NE"] == 2 and drop[1]["nw_bwd"] == 3
    assert drop[2]["nw_bwd"] == 1 and drop[2]["FP"] == 48 and DROP[2][2] > 16
    assert all(qs[n]["trips_bwd"] == 3 for n in BITS[:2]) and qs[BITS[2]]["nw_bwd"] == 3


@functools.lru_cache(maxsize=None)
def make(name):
    return fa.make_case(*CASES[name][0])


@functools.lru_cache(maxsize=None)
def refs(name):
    """(float64, the fp32 composition on the CPU) of a case, computed once."""
    return fa.reference(make(name)), fa.ref32(make(name))


# ---- the tests -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(autouse=True)
def _whole_range(monkeypatch):
    """The kernels over their whole range, whatever the default routing."""
    from recbox_amd import ops
    monkeypatch.setattr(ops.config, "field_attn_fused", True)
    monkeypatch.setattr(ops.config, "field_attn_fields", ops.FIELD_ATTN_MAX_FIELDS)
    monkeypatch.setattr(ops.config, "field_attn_dim", ops.FIELD_ATTN_MAX_DIM)


def _fused_only(monkeypatch):
    """From here on the composition fails the test (``ref32`` IS the composition, so the references are taken before this);
    returns the list that counts the calls reaching rbx_fieldattn_fwd."""
    from recbox_amd import ops
    monkeypatch.setattr(ops, "field_attn_torch", lambda *a, **k: pytest.fail("the fused layer did not run"))
    calls = []
    fwd = ops.lib.rbx_fieldattn_fwd
    monkeypatch.setattr(ops.lib, "rbx_fieldattn_fwd", lambda *a: (calls.append(1), fwd(*a))[1])
    return calls


def _fused(*a):
    from recbox_amd import ops
    return ops.field_attn(*a)


def _check(got, want, ref32, what):
    for n in ALL:
        if want[n] is None:
            assert got[n] is None, n
        else:
            fp32_bar.assert_bar("%s %s" % (n, what), got[n], want[n], ref32[n])


def _same_bits(a, b, what):
    for n in ALL:
        if a[n] is None or b[n] is None:
            assert a[n] is None and b[n] is None, n
        else:
            assert torch.equal(a[n], b[n]), "%s %s" % (what, n)


def test_the_list_covers_every_form():
    check_the_list_covers_every_form()


@pytest.mark.parametrize("name", list(CASES))
def test_form_matches_float64_under_the_fp32_bar(name, monkeypatch):
    q = check_forms(name)
    print("%s: %s" % (name, ", ".join("%s %d" % kv for kv in sorted(q.items()))))
    want, ref32 = refs(name)
    calls = _fused_only(monkeypatch)
    got = fa.run(_fused, make(name), "cuda")
    assert len(calls) == 1
    _check(got, want, ref32, name)


@pytest.mark.parametrize("B,F,E,h", DROP)
def test_dropout_equals_the_restatement_under_the_kernels_mask(B, F, E, h, monkeypatch):
    """p = 0.25 with a fixed seed: the fused layer equals the float64 restatement under
    ops.attention_dropout_mask(B h, F, F, p, seed), same bar; a second run with the seed gives the same bits."""
    from recbox_amd import ops
    p, seed = 0.25, 20261021
    case = fa.make_case(B, F, E, h, True, True, True, p)
    keep = ops.attention_dropout_mask(B * h, F, F, p, seed)
    want, ref32 = fa.reference(case, keep), fa.ref32(case, keep)
    calls = _fused_only(monkeypatch)
    got = fa.run(_fused, case, "cuda", seed=seed)
    _check(got, want, ref32, "dropout-F%d-E%d-h%d" % (F, E, h))
    _same_bits(got, fa.run(_fused, case, "cuda", seed=seed), "same seed")
    assert len(calls) == 2


@pytest.mark.parametrize("name", BITS)
def test_two_runs_give_the_same_bits(name, monkeypatch):
    q = check_forms(name)
    assert q["trips_bwd"] == 3 or q["nw_bwd"] == 3
    calls = _fused_only(monkeypatch)
    _same_bits(fa.run(_fused, make(name), "cuda"), fa.run(_fused, make(name), "cuda"), name)
    assert len(calls) == 2


def test_report_worst_ratio():
    """Prints the worst err / bar per tensor over this module (profiles/autoint/INDEX.md quotes it)."""
    fp32_bar.report("autoint forms")
