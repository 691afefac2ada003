"""The interaction and row-scoring kernels behind the embedding lookup (rbx_interaction.hip, rbx_tower.hip's l2norm /
pairdot, rbx_pool.hip) through their public wrappers, forward and backward, every element against the float64
restatement of oracle/interact64.py with the bound |got - want| <= C eps32 A + tiny (C per op as derived there; the
one-product outputs are compared for equality; A = 0 means exactly zero).

Which instantiation a dim selects.  fm_fwd_kernel / fm_bwd_kernel<G, NV, VEC> (modes 0 / 1): units = D / 4 when
D % 4 == 0, the block and the output are 16-byte aligned and the batch strides are multiples of 4 floats, else D;
G = min(64, next power of two >= units), NV = that power of two / 64 beyond:
  D (float4)              <G, NV, VEC>        D (scalar)   <G, NV, VEC>
  4                       <1, 1, true>        1            <1, 1, false>
  8                       <2, 1, true>        2            <2, 1, false>
  12, 16                  <4, 1, true>        3            <4, 1, false>
  20, 32                  <8, 1, true>        7            <8, 1, false>
  36, 64                  <16, 1, true>       10           <16, 1, false>
  68, 100, 128            <32, 1, true>       17           <32, 1, false>
  132, 192, 252, 256      <64, 1, true>       33, 63       <64, 1, false>
  260, 384, 512           <64, 2, true>       65, 127      <64, 2, false>
  516, 1000, 1024         <64, 4, true>       129, 255     <64, 4, false>
  1028                    refused             257          refused (NotImplementedError, RBX_ERR_UNSUPPORTED)
A float4 dim on a misaligned view (storage offset of one float, or a batch stride that is not a multiple of 4) runs the
scalar form of the same D up to 256; beyond, where no scalar form exists, ops.interaction copies the block to an aligned
buffer (it raised before this file).  fm_sum_fwd_kernel<G>: G = next power of two >= D / 4, D % 4 == 0, D <= 256.
Modes 2 / 3 and pair_mul: one wavefront per sample, the [F, D] block(s) in LDS, refused beyond 64 KB.  With one field the
pairwise outputs are empty and the C entry points write the zero gradients themselves (rbx_interaction_bwd launches the
kernel, whose j loop skips j == i; rbx_pairmul_bwd clears): both returned "NULL tensor" for the empty output before.
l2norm / pairdot / pool<G>: G = min(64, next power of two >= D), a lane walks ceil(D / G) elements.

l2_normalize at magnitudes whose squares leave float32 (pinned in test_l2_normalize_extreme_magnitudes): rows of 1e-20
have a norm below eps in float64 too, so y = x / eps within the bound; rows of 2e18 at D = 16 (sum of squares finite)
meet the bound; at D = 1000 the sum of squares is inf and y = 0 exactly -- which is what F.normalize returns in float32
(its norm is inf as well), so the kernel is not changed.

Worst err / bound achieved on the MI355X (202 cases, 42 s; every op below 0.12 of its bound, so nothing near 0.5):
  modes 0 / 1, every <G, NV, VEC>   forward 0.083 (<64, 4, true>, one-signed bi_interaction), gradient 0.068; randn below 0.04
  modes 2 / 3                       inner_product 0.064, gradients 0.094 (spread inputs); elementwise_product equal
  pair_mul                          forward and per-pair dleft equal; per-field dleft 0.063, dright 0.064
  fm_sum<G> (DeepFM input stage)    y_fm 0.0098, y_lr 0.017; the block's gradient 0.027 of (GEMM tolerance + fm bound)
  l2norm<G>                         forward 0.028, backward 0.048;  pairdot<G>: forward 0.028, du 0.114 (N = 101 candidates
                                    summed in sequence, D = 2049), dv 0.015;  pool<G>: forward 0.048, backward 0.015
The kernel-level cases (rbx_interaction_bwd's strided store into a NaN-filled wider buffer: 0.033; modes 2 / 3 on a
storage-offset view: 0.043) and DeepFM as a model where supported() is False (dim 6, dim 260, a misaligned block; dim 8
as the fused control: predictions and gradients below 0.01 of their tolerances) stay inside the same figures.
Mutation check (a scratch build, not kept): with the last live unit of mode 1's store dropped for NV > 1 and field F - 1
skipped in pair_bwd_kernel for F > 6 (at F = 6 the inner_product fixture compares that gradient), the 519 GPU tests that
existed before this file all still passed; 31 cases of this file failed (D = 260 .. 1024 and scalar 65 .. 255 in every
mode 1 test, modes 2 / 3 from F = 39 on).  B = 5000 in mode 3 only where its [B, P, D] output stays small
(F D <= 195); mode 2 alone runs it up to (40, 100), not at (64, 256)."""
import pytest
import torch

from conftest import _note
from oracle import interact64 as I
from test_interact64_restatement import KINDS, one_signed, randn, spread, value_safe

pytestmark = pytest.mark.gpu

VEC = [4, 8, 12, 16, 20, 32, 36, 64, 68, 100, 128, 132, 192, 252, 256, 260, 384, 512, 516, 1000, 1024]
SCALAR = [1, 2, 3, 7, 10, 17, 33, 63, 65, 127, 129, 255]
ROW_DIMS = [1, 2, 3, 7, 16, 33, 64, 65, 100, 128, 200, 256, 1000, 1024, 2049]
FIELDS = [1, 2, 3, 4, 5, 6, 39, 40]
MODES = {0: "product_sum", 1: "bi_interaction", 2: "inner_product", 3: "elementwise_product"}


def form(D, vec=None):
    vec = (D % 4 == 0) if vec is None else vec
    units = D // 4 if vec else D
    g = I.lane_group(units)
    nv = 1 if units <= 64 else (2 if units <= 128 else 4)
    return "fm<%d, %d, %s>" % (g, nv, "true" if vec else "false")


class Worst(object):
    """Collects max(err / bound) per label; ``close`` notes them in the ledger and asserts."""

    def __init__(self):
        self.worst, self.where = {}, {}

    def add(self, label, tag, got, want, A, C):
        assert tuple(got.shape) == tuple(want.shape), "%s: shape %s, expected %s" % (tag, tuple(got.shape), tuple(want.shape))
        got = got.detach().double().cpu()
        if want.numel() == 0:
            return
        assert bool(torch.isfinite(got).all()), "%s: %s is not finite" % (tag, label)
        zero = A == 0
        assert int(torch.count_nonzero(got[zero])) == 0, "%s: %s is not exactly zero where A = 0" % (tag, label)
        r = float(I.ratios(got, want, A, C).max())
        if r > self.worst.get(label, -1.0):
            self.worst[label], self.where[label] = r, tag

    def equal(self, label, tag, got, want):
        assert tuple(got.shape) == tuple(want.shape), tag
        bad = int((got.detach().double().cpu() != want).sum())
        assert bad == 0, "%s: %s: %d elements differ from the float32 product" % (tag, label, bad)

    def close(self):
        for label, r in sorted(self.worst.items()):
            _note(label + " (err / bound)", r, 1.0)
        print("; ".join("%s %.3g" % kv for kv in sorted(self.worst.items())))
        bad = ["%s: %.3g x the bound at %s" % (k, r, self.where[k]) for k, r in sorted(self.worst.items()) if r > 1.0]
        assert not bad, "\n".join(bad)


def _interact(view_of, base, mode, g):
    """ops.interaction on ``view_of(base)`` (base a leaf on the GPU); returns (out, gradient of base)."""
    from recbox_amd import ops
    base = base.detach().requires_grad_(True)
    out = ops.interaction(view_of(base), MODES[mode])
    out.backward(g)
    torch.cuda.synchronize()
    return out.detach(), base.grad


def _modes01(w, label, tag, e, base, view_of, grad_of, seed, modes=(0, 1), kind=randn):
    """Both modes on one block: e [B, F, D] on the CPU is what ``view_of(base)`` shows; grad_of(base.grad) -> [B, F, D]."""
    B, F, D = e.shape
    bi, a_bi = I.bi_interaction64(e)
    for mode in modes:
        want, A = (bi.sum(1, keepdim=True), a_bi.sum(1, keepdim=True)) if mode == 0 else (bi, a_bi)
        g = kind(tuple(want.shape), seed + mode)
        out, grad = _interact(view_of, base, mode, g.cuda())
        t = "%s F%d B%d %s" % (tag, F, B, MODES[mode])
        w.add("%s %s" % (label, MODES[mode]), t, out, want, A, I.c_fm_fwd(F))
        gw, gA = I.fm_grad64(e, g)
        w.add("%s %s gradient" % (label, MODES[mode]), t, grad_of(grad), gw, gA, I.c_fm_bwd(F))
    return w


def _plain(e):
    return e.cuda(), (lambda b: b), (lambda g: g)


# ---- modes 0 / 1: every form ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", VEC + SCALAR)
def test_fm_modes_at_every_form_against_float64(D):
    """F in 1 .. 6, 39, 40 x B in 1, 7, 257 x product_sum and bi_interaction, randn inputs; F = 200 at D = 16 and 100."""
    w = Worst()
    for F in FIELDS + ([200] if D in (16, 100) else []):
        for B in (1, 7, 257):
            e = randn((B, F, D), D * 1000 + F * 10 + B)
            _modes01(w, form(D), "D%d" % D, e, *_plain(e), seed=D + F + B)
    w.close()


@pytest.mark.parametrize("kind", ["one_signed", "spread"])
@pytest.mark.parametrize("D", [4, 8, 16, 32, 64, 128, 256, 512, 1024, 1, 2, 3, 7, 10, 17, 33, 65, 129])
def test_fm_modes_on_one_signed_and_spread_inputs(D, kind):
    """One D per form on the inputs where a biased or mis-ordered sum shows: all positive of one magnitude, and mixed sign
    spread over e^+-6."""
    w = Worst()
    for F in (2, 5, 39, 200):
        e = KINDS[kind]((61, F, D), D + F)
        _modes01(w, "%s %s" % (form(D), kind), "D%d" % D, e, *_plain(e), seed=D * F, kind=KINDS[kind])
    w.close()


@pytest.mark.parametrize("how", ["offset", "stride"])
@pytest.mark.parametrize("D", [4, 16, 64, 100, 132, 256])
def test_fm_modes_scalar_form_forced_at_a_float4_dim(D, how):
    """D % 4 == 0 read through a view whose storage offset is one float, and through a batch stride with sb % 4 == 1."""
    w = Worst()
    for F in (1, 3, 6, 39):
        for B in (1, 7, 257):
            e = randn((B, F, D), D * 77 + F + B)
            if how == "offset":
                base = torch.zeros(B * F * D + 1)
                base[1:] = e.reshape(-1)
                view_of = lambda b: b[1:].view(B, F, D)                               # noqa: E731
                grad_of = lambda g: g[1:].view(B, F, D)                               # noqa: E731
                assert B * F * D == 0 or (base.cuda()[1:].data_ptr() % 16) != 0
            else:
                base = torch.full((B, F * D + 5), float("nan"))
                base[:, :F * D] = e.reshape(B, -1)
                view_of = lambda b: b[:, :F * D].view(B, F, D)                        # noqa: E731
                grad_of = lambda g: g[:, :F * D].reshape(B, F, D)                     # noqa: E731
            _modes01(w, form(D, vec=False) + " forced", "D%d %s" % (D, how), e, base.cuda(), view_of, grad_of, seed=D + F)
    w.close()


@pytest.mark.parametrize("G,F,D,B", [(1, 2, 1, 2048 * 256 + 5), (4, 3, 16, 2048 * 64 + 37), (64, 2, 256, 2048 * 4 + 37),
                                     ("64 NV4", 2, 1024, 2048 * 4 + 37)])
def test_fm_modes_grid_stride_loop_takes_a_second_ragged_trip(G, F, D, B):
    """The grid is capped at 2048 workgroups of 256 / G groups: B just past that, so every group iterates and the second
    trip is mostly empty."""
    w = Worst()
    e = randn((B, F, D), B)
    _modes01(w, form(D) + " past the cap", "D%d" % D, e, *_plain(e), seed=B)
    w.close()


@pytest.mark.parametrize("k", [4, 3])
@pytest.mark.parametrize("D", [4, 16, 100, 256, 1024])
def test_fm_modes_read_a_block_in_place_inside_a_wider_row(D, k):
    """[B, F, D] as the leading columns of [B, F D + k], the trailing columns NaN: k = 4 keeps the float4 form, k = 3 makes
    the batch stride odd (scalar form; beyond D = 256 an aligned copy).  The outputs stay finite, the block's gradient is
    [B, F, D] (the wrapper's gradient is a tight tensor of its own; autograd's slice pads the zeros).  The kernel's own
    strided store is seen through rbx_interaction_bwd called directly on a NaN-filled [B, F D + k] buffer (dsb = F D + k):
    the block meets the bound and every trailing column is still NaN.  The C entry point has no copy to fall back on:
    k = 3 at D = 1024 is refused there."""
    import ctypes
    from recbox_amd import _lib
    w = Worst()
    for F in (1, 5, 39):
        B = 61
        e = randn((B, F, D), D + F + k + 1)
        wide = torch.full((B, F * D + k), float("nan"))
        wide[:, :F * D] = e.reshape(B, -1)
        wide = wide.cuda()
        for mode in (0, 1):
            g = randn((B, 1 if mode == 0 else D), F + mode)
            gc = g.cuda()
            demb = torch.full((B, F * D + k), float("nan"), device="cuda")
            rc = _lib.lib.rbx_interaction_bwd(ctypes.c_void_p(wide.data_ptr()), F * D + k, ctypes.c_void_p(gc.data_ptr()), B, F, D,
                                              mode, ctypes.c_void_p(demb.data_ptr()), F * D + k, None)
            torch.cuda.synchronize()
            if k == 3 and D > 256:
                assert rc == _lib.RBX_ERR_UNSUPPORTED and bool(torch.isnan(demb).all())
                continue
            _lib.check(rc)
            assert bool(torch.isnan(demb[:, F * D:]).all()), "D%d k%d F%d: the backward wrote beyond the block" % (D, k, F)
            w.add("fm strided store %s gradient" % MODES[mode], "D%d k%d F%d" % (D, k, F), demb[:, :F * D].reshape(B, F, D),
                  *I.fm_grad64(e, g), I.c_fm_bwd(F))
    for F in (1, 5, 39):
        B = 61
        e = randn((B, F, D), D + F + k)
        base = torch.full((B, F * D + k), float("nan"))
        base[:, :F * D] = e.reshape(B, -1)
        tails = []

        def grad_of(g):
            tails.append(g[:, F * D:])
            return g[:, :F * D].reshape(B, F, D)

        label = (form(D) if k == 4 else (form(D, vec=False) if D <= 256 else form(D) + " copied")) + " in place"
        _modes01(w, label, "D%d k%d" % (D, k), e, base.cuda(), lambda b: b[:, :F * D].view(B, F, D), grad_of, seed=D + k)
        assert all(int(torch.count_nonzero(t)) == 0 for t in tails)
    w.close()


@pytest.mark.parametrize("D", [257, 1028])
def test_fm_dims_without_a_form_are_refused(D):
    from recbox_amd import ops
    e = randn((5, 3, D), D).cuda()
    for mode in ("product_sum", "bi_interaction"):
        with pytest.raises(NotImplementedError, match="interaction dim too large"):
            ops.interaction(e, mode)
    torch.cuda.synchronize()
    e = randn((5, 3, 4), 1)                                               # ... and the next call runs
    _modes01(Worst(), form(4), "after the refusal", e, *_plain(e), seed=1).close()


@pytest.mark.parametrize("D", [260, 512, 1024])
def test_fm_misaligned_view_beyond_the_scalar_forms_is_copied_and_computes(D):
    """A misaligned view at a dim only the float4 forms take (scalar units > 256) is a layout accident: it raised
    'interaction dim too large' before; ops.interaction now reads an aligned copy."""
    w = Worst()
    B, F = 33, 5
    e = randn((B, F, D), D)
    base = torch.zeros(B * F * D + 1)
    base[1:] = e.reshape(-1)
    _modes01(w, form(D) + " copied", "D%d offset" % D, e, base.cuda(), lambda b: b[1:].view(B, F, D),
             lambda g: g[1:].view(B, F, D), seed=D)
    w.close()


def test_interaction_modules_against_float64():
    """layers.InnerProductInteraction in its four outputs and rechub FM (reduce_sum or not) map onto the same kernels."""
    from recbox_amd.ranking.pytorch import layers as L
    from recbox_amd.rechub.basic import layers as hub
    w = Worst()
    B, F, D = 257, 39, 100
    e = randn((B, F, D), 5)
    mods = [(L.InnerProductInteraction(F, "product_sum"), I.product_sum64, I.fm_grad64, I.c_fm_fwd(F), I.c_fm_bwd(F)),
            (L.InnerProductInteraction(F, "bi_interaction"), I.bi_interaction64, I.fm_grad64, I.c_fm_fwd(F), I.c_fm_bwd(F)),
            (hub.FM(reduce_sum=True), I.product_sum64, I.fm_grad64, I.c_fm_fwd(F), I.c_fm_bwd(F)),
            (hub.FM(reduce_sum=False), I.bi_interaction64, I.fm_grad64, I.c_fm_fwd(F), I.c_fm_bwd(F)),
            (L.InnerProductInteraction(F, "inner_product"), I.inner_product64, I.pair_grad64, I.c_inner(D), I.c_pair_bwd(F)),
            (L.InnerProductInteraction(F, "elementwise_product"), I.elementwise_product64, I.pair_grad64, None, I.c_pair_bwd(F))]
    for n, (mod, fwd, grad, cf, cb) in enumerate(mods):
        ec = e.cuda().requires_grad_(True)
        out = mod.cuda()(ec)
        want, A = fwd(e)
        g = randn(tuple(want.shape), n)
        out.backward(g.cuda())
        torch.cuda.synchronize()
        if cf is None:
            w.equal("modules", "module %d" % n, out, want)
        else:
            w.add("modules forward", "module %d" % n, out, want, A, cf)
        w.add("modules backward", "module %d" % n, ec.grad, *grad(e, g), cb)
    w.close()


# ---- modes 2 / 3 ----------------------------------------------------------------------------------------------------------
def _pairwise(w, label, tag, e, base, view_of, grad_of, seed, kind=randn, modes=(2, 3)):
    B, F, D = e.shape
    for mode, fwd in ((2, I.inner_product64), (3, I.elementwise_product64)):
        if mode not in modes:
            continue
        want, A = fwd(e)
        g = kind(tuple(want.shape), seed + mode)
        out, grad = _interact(view_of, base, mode, g.cuda())
        t = "%s F%d D%d B%d %s" % (tag, F, D, B, MODES[mode])
        if mode == 2:
            w.add(label + " inner_product", t, out, want, A, I.c_inner(D))
        else:
            w.equal(label + " elementwise_product", t, out, want)
        gw, gA = I.pair_grad64(e, g)
        w.add("%s %s gradient" % (label, MODES[mode]), t, grad_of(grad), gw, gA, I.c_pair_bwd(F))


# B = 5000 in both modes only where the mode 3 output ([B, P, D]) stays small; (64, 256) is exactly 64 KB of LDS
PAIR_SHAPES = [(2, 1, (1, 257, 5000)), (3, 2, (1, 257, 5000)), (6, 8, (1, 257, 5000)), (39, 16, (1, 257)), (40, 100, (1, 257)),
               (65, 3, (1, 257, 5000)), (64, 256, (1, 7))]


@pytest.mark.parametrize("F,D,batches", PAIR_SHAPES)
def test_pairwise_modes_against_float64(F, D, batches):
    w = Worst()
    for B in batches:
        e = randn((B, F, D), F * D + B)
        _pairwise(w, "pair", "plain", e, *_plain(e), seed=F + D)
    e = one_signed((7, F, D), F)
    _pairwise(w, "pair one_signed", "one_signed", e, *_plain(e), seed=F, kind=one_signed)
    e = spread((7, F, D), F)
    _pairwise(w, "pair spread", "spread", e, *_plain(e), seed=F, kind=spread)
    if 5000 not in batches and F * D < 16384:                                 # mode 2 alone ([B, P]) fits at B = 5000
        e = randn((5000, F, D), F * D)
        _pairwise(w, "pair", "plain", e, *_plain(e), seed=F + D, modes=(2,))
    B = 61                                                                   # the block inside a wider row, tail NaN
    e = randn((B, F, D), 5)
    base = torch.full((B, F * D + 3), float("nan"))
    base[:, :F * D] = e.reshape(B, -1)
    _pairwise(w, "pair in place", "in place", e, base.cuda(), lambda b: b[:, :F * D].view(B, F, D),
              lambda g: g[:, :F * D].reshape(B, F, D), seed=9)
    base = torch.zeros(B * F * D + 1)                                        # a view whose storage offset is one float
    base[1:] = e.reshape(-1)
    _pairwise(w, "pair offset view", "offset", e, base.cuda(), lambda b: b[1:].view(B, F, D),
              lambda g: g[1:].view(B, F, D), seed=10)
    w.close()


def test_pairwise_modes_beyond_64_kb_of_lds_are_refused():
    from recbox_amd import ops
    e = randn((3, 65, 256), 1).cuda()
    for mode in ("inner_product", "elementwise_product"):
        with pytest.raises(NotImplementedError, match="too large for the pairwise modes"):
            ops.interaction(e, mode)
    torch.cuda.synchronize()


@pytest.mark.parametrize("mode", [2, 3])
def test_pairwise_modes_with_one_field(mode):
    """No pair: the output is empty and the gradient exactly zero -- written by rbx_interaction_bwd itself (called here on a
    NaN-filled buffer, with NULL for the empty upstream gradient), not by the wrapper."""
    import ctypes
    from recbox_amd import _lib
    B, D = 257, 12
    e = randn((B, 1, D), 3)
    out, grad = _interact(lambda b: b, e.cuda(), mode, torch.zeros((B, 0) if mode == 2 else (B, 0, D), device="cuda"))
    assert tuple(out.shape) == ((B, 0) if mode == 2 else (B, 0, D))
    assert tuple(grad.shape) == (B, 1, D) and int(torch.count_nonzero(grad)) == 0
    ec = e.cuda()
    demb = torch.full((B, 1, D), float("nan"), device="cuda")
    _lib.check(_lib.lib.rbx_interaction_bwd(ctypes.c_void_p(ec.data_ptr()), D, None, B, 1, D, mode,
                                            ctypes.c_void_p(demb.data_ptr()), D, None))
    torch.cuda.synchronize()
    assert int(torch.count_nonzero(demb)) == 0


# ---- pair_mul -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_pair", [False, True])
@pytest.mark.parametrize("F,D,batches", [(1, 4, (1, 257)), (2, 1, (1, 257, 5000)), (3, 2, (1, 257, 5000)), (6, 8, (1, 257, 5000)),
                                         (39, 16, (1, 257)), (40, 100, (1, 61)), (65, 3, (1, 257)), (32, 256, (1, 7))])
def test_pair_mul_against_float64(F, D, batches, per_pair):
    """(32, 256): 2 F D floats = exactly 64 KB of LDS.  F = 1: empty output, zero gradients."""
    from recbox_amd import ops
    w = Worst()
    P = F * (F - 1) // 2
    for kind in ("randn", "one_signed", "spread"):
        for B in (batches if kind == "randn" else batches[:1] + (7,)):
            right, left, g = (KINDS[kind](s, F + D + B + n) for n, s in enumerate(((B, F, D), (B, P if per_pair else F, D), (B, P, D))))
            lc, rc = left.cuda().requires_grad_(True), right.cuda().requires_grad_(True)
            out = ops.pair_mul(lc, rc, per_pair)
            out.backward(g.cuda())
            torch.cuda.synchronize()
            t = "F%d D%d B%d %s" % (F, D, B, kind)
            w.equal("pair_mul", t, out, I.pair_mul64(left, right, per_pair)[0])
            (dl, al), (dr, ar) = I.pair_mul_grad64(left, right, g, per_pair)
            if per_pair:
                w.equal("pair_mul per pair dleft", t, lc.grad, dl)
            else:
                w.add("pair_mul per field dleft", t, lc.grad, dl, al, I.c_pair_bwd(F))
            w.add("pair_mul %s dright" % ("per pair" if per_pair else "per field"), t, rc.grad, dr, ar, I.c_pair_bwd(F))
    w.close()


@pytest.mark.parametrize("per_pair", [0, 1])
def test_pair_mul_backward_with_one_field_writes_its_zeros(per_pair):
    """rbx_pairmul_bwd called directly on NaN-filled gradients with F = 1 (the upstream gradient and a per-pair left are
    empty: NULL): dright, and the per-field dleft, come back exactly zero.  The wrapper allocates them uninitialised."""
    import ctypes
    from recbox_amd import _lib
    B, D = 257, 12
    x = randn((B, 1, D), 1).cuda()
    dleft = torch.full((B, 1, D), float("nan"), device="cuda")
    dright = torch.full((B, 1, D), float("nan"), device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())                              # noqa: E731
    _lib.check(_lib.lib.rbx_pairmul_bwd(None if per_pair else p(x), p(x), None, B, 1, D, per_pair,
                                        None if per_pair else p(dleft), p(dright), None))
    torch.cuda.synchronize()
    assert int(torch.count_nonzero(dright)) == 0
    assert bool(torch.isnan(dleft).all()) if per_pair else int(torch.count_nonzero(dleft)) == 0


def test_pair_mul_beyond_64_kb_of_lds_is_refused():
    from recbox_amd import ops
    x = randn((3, 33, 256), 1).cuda()
    with pytest.raises(NotImplementedError, match="pairmul: F\\*D=8448 too large"):
        ops.pair_mul(x, x, False)
    torch.cuda.synchronize()


# ---- DeepFM's input stage -----------------------------------------------------------------------------------------------------
def _deepfm_case(w, dim, F, dense, padded, fuse_lr, M, N=32):
    """h, y_fm, y_lr and every gradient of ops.deepfm_input_stage against float64.  fm_sum's parts (y_fm, y_lr) use the
    restatement's bounds; the GEMM parts (h, dW1, db1, and the first-order head's dw / db, which run the n = 1 linear
    backward) keep test_linear_matches_torch_fp32's tolerances on inputs scaled as there; the block's gradient is the sum
    dh W1 + g_fm (S - e) + g_lr w_lr: the GEMM's tolerance plus the restatement's bound on the other two terms."""
    from recbox_amd import ops
    K = F * dim + dense
    gen = torch.Generator().manual_seed(dim * 1000 + F * 10 + dense + M)
    x = torch.randn(M, K, generator=gen)
    lin1, lr = torch.nn.Linear(K, N), torch.nn.Linear(F * dim, 1)
    with torch.no_grad():
        lin1.weight.copy_(torch.randn(N, K, generator=gen) / K ** 0.5)
        lin1.bias.copy_(torch.randn(N, generator=gen))
        lr.weight.copy_(torch.randn(1, F * dim, generator=gen) / (F * dim) ** 0.5)
        lr.bias.copy_(torch.randn(1, generator=gen))
    dh, gf, gl = torch.randn(M, N, generator=gen), torch.randn(M, 1, generator=gen), torch.randn(M, 1, generator=gen)
    lin1c, lrc = torch.nn.Linear(K, N).cuda(), torch.nn.Linear(F * dim, 1).cuda()
    lin1c.load_state_dict(lin1.state_dict())
    lrc.load_state_dict(lr.state_dict())
    if padded:
        Kp = (K + 3) // 4 * 4 + 4
        base = torch.full((M, Kp), float("nan"), device="cuda")
        base[:, :K] = x.cuda()
        base.requires_grad_(True)
        xc = base[:, :K]
    else:
        base = x.cuda().requires_grad_(True)
        xc = base
    assert ops.deepfm_input_stage_supported(xc, F * dim, dim), "dim%d F%d dense%d padded=%s refused" % (dim, F, dense, padded)
    old = ops.config.fuse_deepfm_lr
    ops.config.fuse_deepfm_lr = fuse_lr
    try:
        h, y_fm, y_lr = ops.deepfm_input_stage(xc, lin1c, lrc, F * dim, dim)
        torch.autograd.backward([h, y_fm, y_lr], [dh.cuda(), gf.cuda(), gl.cuda()])
        ops.join_beside()
        torch.cuda.synchronize()
    finally:
        ops.config.fuse_deepfm_lr = old
    tag = "dim%d F%d dense%d padded=%s fuse_lr=%s M%d" % (dim, F, dense, padded, fuse_lr, M)
    parts = I.fm_sum64(x, F, dim, lr.weight, lr.bias)
    w.add("fm_sum<%d> y_fm" % I.lane_group(dim // 4), tag, y_fm, *parts["y_fm"], I.c_fm_fwd(F))
    if fuse_lr:
        w.add("fm_sum<%d> y_lr" % I.lane_group(dim // 4), tag, y_lr, *parts["y_lr"], I.c_fm_fwd(F))
    x64, W64, b64 = x.double(), lin1.weight.detach().double(), lin1.bias.detach().double()

    def close(what, got, want, tol):
        err = float((got.detach().double().cpu().reshape(want.shape) - want).abs().max())
        _note("deepfm_input_stage " + what, err, tol)
        assert err <= tol, "%s: %s error %.3e > %.1e" % (tag, what, err, tol)

    close("h", h, x64 @ W64.t() + b64, 2e-5 * max(1.0, K ** 0.5 / 8))
    if not fuse_lr:
        close("y_lr", y_lr, parts["y_lr"][0], 2e-5 * max(1.0, (F * dim) ** 0.5 / 8))
    scale = 1e-4 * max(1.0, M ** 0.5 / 16)
    close("dW1", lin1c.weight.grad, dh.double().t() @ x64, scale)
    close("db1", lin1c.bias.grad, dh.double().sum(0), scale)
    close("dw_lr", lrc.weight.grad, gl.double().t() @ x64[:, :F * dim], scale)
    close("db_lr", lrc.bias.grad, gl.double().sum(0), scale)
    e = x[:, :F * dim].reshape(M, F, dim)
    fm, a_fm = I.fm_grad64(e, gf)
    lw = gl.double() * lr.weight.detach().double()
    want = dh.double() @ W64
    want[:, :F * dim] += fm.reshape(M, -1) + lw
    tol = torch.full((M, K), 1e-4, dtype=torch.float64)
    tol[:, :F * dim] += I.EPS32 * (I.c_fm_bwd(F) * a_fm.reshape(M, -1) + I.C_BOUND * lw.abs())
    got = base.grad.detach().double().cpu()
    if padded:
        assert int(torch.count_nonzero(got[:, K:])) == 0, tag
        got = got[:, :K]
    r = float(((got - want).abs() / tol).max())
    _note("deepfm_input_stage dx (err / (GEMM tolerance + fm bound))", r, 1.0)
    assert r <= 1.0, "%s: dx is %.3g x its tolerance" % (tag, r)
    return True


@pytest.mark.parametrize("dim", [4, 8, 12, 16, 32, 64, 100, 128, 132, 256])
def test_deepfm_input_stage_at_every_dim_against_float64(dim):
    w = Worst()
    ran = 0
    for F in (1, 3, 26, 39):
        for dense in (0, 1, 13):
            for padded in (False, True):
                if not padded and (F * dim + dense) % 4 != 0:
                    continue                                              # an unpadded row stride must be a multiple of 4 floats
                for fuse_lr in (True, False):
                    ran += bool(_deepfm_case(w, dim, F, dense, padded, fuse_lr, 300))
    assert ran == 32          # 4 F x (dense 0: padded or not; dense 1, 13: padded) x fuse_lr on / off, every one supported()
    w.close()


def test_deepfm_input_stage_past_the_grid_cap():
    w = Worst()
    assert _deepfm_case(w, 256, 3, 13, True, True, 2048 * 4 + 37)
    assert _deepfm_case(w, 16, 3, 13, True, True, 2048 * 64 + 37)
    w.close()


def test_deepfm_input_stage_unsupported_side():
    from recbox_amd import ops
    x = torch.zeros(8, 64, device="cuda")
    assert ops.deepfm_input_stage_supported(x, 48, 16)
    assert not ops.deepfm_input_stage_supported(x, 48, 6)                 # dim % 4
    assert not ops.deepfm_input_stage_supported(torch.zeros(8, 2 * 260 + 4, device="cuda"), 520, 260)
    assert not ops.deepfm_input_stage_supported(torch.zeros(8, 65, device="cuda")[:, 1:], 48, 16)      # misaligned block
    assert not ops.deepfm_input_stage_supported(torch.zeros(8, 63, device="cuda"), 48, 16)             # odd row stride


@pytest.mark.parametrize("dim,misaligned,fused", [(8, False, True), (6, False, False), (260, False, False), (8, True, False)])
def test_deepfm_model_falls_back_where_the_input_stage_is_unsupported_and_still_matches(dim, misaligned, fused):
    """rechub DeepFM (the caller that branches on deepfm_input_stage_supported) at dim 6 (dim % 4), dim 260 (> 256) and on a
    gathered block that is not 16-byte aligned (the embedding layer's output re-laid one float into a buffer, row stride
    F dim + 3), with dim 8 on the aligned block as the control that does take the fused stage.  Whether the stage ran is
    observed; predictions and every gradient are compared with oracle.torch_ref.RefDeepFM in float64.  The tower is its
    output Linear alone (no ReLU whose kink float32 and float64 could take differently).  Tolerances: the logit is
    y_lr + y_fm + y_deep, so |d logit| <= c_fm_fwd(F) eps32 A(y_fm) + the GEMM's forward tolerance
    (test_linear_matches_torch_fp32's) for each of the two Linears, and a probability moves by at most a quarter of that;
    dense gradients keep that test's dw / db tolerance; a table row's gradient is a sum of its lookups' dx rows, each at
    that test's dx tolerance of 1e-4."""
    from oracle import torch_ref as R
    from recbox_amd import ops
    from recbox_amd.rechub.basic.features import DenseFeature, SparseFeature
    from recbox_amd.rechub.models.ranking import DeepFM
    B, F = 300, 3
    gen = torch.Generator().manual_seed(dim + int(misaligned))
    sparse = [SparseFeature("C%d" % i, 40 + 7 * i, dim) for i in range(F)]
    dense = [DenseFeature("I%d" % i) for i in range(3)]
    mlp = {"dims": [], "dropout": 0.0, "activation": "relu"}
    model = DeepFM(sparse + dense, sparse, mlp)
    with torch.no_grad():
        for name, p in model.named_parameters():
            p.copy_(torch.randn(p.shape, generator=gen) * (dim ** -0.5 if "embed" in name else p.shape[-1] ** -0.5))
    ref = R.RefDeepFM(sparse + dense, sparse, mlp).double()
    ref.load_state_dict({k: (v.double() if v.is_floating_point() else v) for k, v in model.state_dict().items()})
    model.cuda().train()
    ref.train()
    x = {f.name: torch.randint(0, f.vocab_size, (B,), generator=gen) for f in sparse}
    x.update({f.name: torch.rand(B, generator=gen) for f in dense})
    if misaligned:
        aligned_forward = model.embedding.forward

        def shifted(xin, features, squeeze_dim=False):
            out = aligned_forward(xin, features, squeeze_dim=squeeze_dim)
            if not squeeze_dim:
                return out
            flat = torch.cat([out.new_zeros(1), out.reshape(-1)])
            out = flat[1:].view(out.shape)
            assert out.data_ptr() % 16 != 0
            return out

        model.embedding.forward = shifted
    calls = []
    real_stage = ops.deepfm_input_stage

    def counting_stage(*args):
        calls.append(1)
        return real_stage(*args)

    ops.deepfm_input_stage = counting_stage
    Rn = torch.randn(B, generator=gen)
    try:
        pred = model({k: v.cuda() for k, v in x.items()})
        (pred * Rn.cuda()).sum().backward()
        ops.join_beside()
        torch.cuda.synchronize()
    finally:
        ops.deepfm_input_stage = real_stage
    assert len(calls) == (1 if fused else 0), "the fused input stage ran %d times" % len(calls)
    xs = {k: (v.double() if v.is_floating_point() else v) for k, v in x.items()}
    want = ref(xs)
    (want * Rn.double()).sum().backward()
    e = ref.embedding(xs, sparse, squeeze_dim=False).detach()
    _, a_fm = I.product_sum64(e)
    K = F * dim + len(dense)
    tol = 0.25 * (I.c_fm_fwd(F) * I.EPS32 * a_fm.view(-1) + 2e-5 * max(1.0, K ** 0.5 / 8) + 2e-5 * max(1.0, (F * dim) ** 0.5 / 8))
    r = float(((pred.detach().double().cpu() - want.detach()).abs() / tol).max())
    _note("DeepFM dim %d%s prediction (err / tolerance)" % (dim, " misaligned" if misaligned else ""), r, 1.0)
    assert r <= 1.0, "prediction is %.3g x its tolerance" % r
    got = dict(model.named_parameters())
    for name, p in ref.named_parameters():
        g = got[name].grad.detach().double().cpu()
        if "embed" in name:
            feat = [f for f in sparse if ("." + f.name + ".") in name][0]
            count = torch.bincount(x[feat.name], minlength=p.shape[0]).double().clamp_min(1.0)
            tol_p = (1e-4 * count).view(-1, 1)
        else:
            tol_p = torch.tensor(1e-4 * max(1.0, B ** 0.5 / 16), dtype=torch.float64)
        r = float(((g - p.grad).abs() / tol_p).max())
        _note("DeepFM dim %d%s grad %s (err / tolerance)" % (dim, " misaligned" if misaligned else "", name), r, 1.0)
        assert r <= 1.0, "grad %s is %.3g x its tolerance" % (name, r)
        assert float(p.grad.abs().max()) > 1e-3, name                       # the comparison is not between zeros


# ---- l2_normalize ---------------------------------------------------------------------------------------------------------------
def _l2(w, label, tag, x, view_of=None, base=None, kind=randn, eps=1e-12):
    from recbox_amd import ops
    dy = kind(tuple(x.shape), x.numel() % 1000 + 3)
    base = (x.cuda() if base is None else base).detach().requires_grad_(True)
    y = ops.l2_normalize(view_of(base) if view_of else base, eps)
    y.backward(dy.cuda())
    torch.cuda.synchronize()
    D = x.shape[-1]
    want, A, _ = I.l2_normalize64(x, eps)
    w.add(label + " forward", tag, y, want, A, I.c_rows(D))
    gw, gA = I.l2_normalize_grad64(x, dy, eps)
    return base.grad, gw, gA


@pytest.mark.parametrize("D", ROW_DIMS)
def test_l2_normalize_against_float64(D):
    w = Worst()
    label = "l2norm<%d>" % I.lane_group(D)
    for kind in ("randn", "one_signed", "spread"):
        for shape in ((1, D), (257, D), (5, 7, D)):
            x = KINDS[kind](shape, D + len(shape))
            if shape[0] == 257:
                x[3] = 0                                                   # A = 0: exactly zero both ways
                x[5] *= 1e-14 / max(1.0, float(x[5].abs().max()))          # norm below eps: the clamped branch
            g, gw, gA = _l2(w, label, "D%d %s %s" % (D, kind, shape), x, kind=KINDS[kind])
            w.add(label + " backward", "D%d %s %s" % (D, kind, shape), g, gw, gA, I.c_rows(D))
    B, n = 33, 3                                                          # [B, n, D] behind 5 leading columns: read in place
    x = randn((B, n, D), D)
    base = torch.full((B, 5 + n * D), float("nan"))
    base[:, 5:] = x.reshape(B, -1)
    g, gw, gA = _l2(w, label + " strided", "D%d strided" % D, x, lambda b: b[:, 5:].view(B, n, D), base.cuda())
    assert int(torch.count_nonzero(g[:, :5])) == 0
    w.add(label + " strided backward", "D%d strided" % D, g[:, 5:].reshape(B, n, D), gw, gA, I.c_rows(D))
    w.close()


@pytest.mark.parametrize("D,rows", [(1, 2048 * 256 + 5), (16, 2048 * 16 + 37), (256, 2048 * 4 + 37)])
def test_l2_normalize_past_the_grid_cap(D, rows):
    w = Worst()
    label = "l2norm<%d> past the cap" % I.lane_group(D)
    x = randn((rows, D), D)
    g, gw, gA = _l2(w, label, "D%d rows%d" % (D, rows), x)
    w.add(label + " backward", "D%d" % D, g, gw, gA, I.c_rows(D))
    w.close()


def test_l2_normalize_extreme_magnitudes():
    """What the unscaled sum of squares does where the squares leave float32, pinned (see the header): 1e-20 rows are
    clamped in float64 too and meet the bound; 2e18 rows meet it while the sum of squares is finite (D = 16) and come out
    exactly zero where it is inf (D = 1000) -- as F.normalize does in float32, whose norm is inf there as well."""
    import torch.nn.functional as F_
    from recbox_amd import ops
    w = Worst()
    for D in (16, 1000):
        small = one_signed((9, D), D) * 1e-20
        g, gw, gA = _l2(w, "l2norm 1e-20", "D%d 1e-20" % D, small, kind=one_signed)
        w.add("l2norm 1e-20 backward", "D%d" % D, g, gw, gA, I.c_rows(D))
    big = one_signed((9, 16), 1) * 2e18
    g, gw, gA = _l2(w, "l2norm 2e18", "D16 2e18", big, kind=one_signed)
    w.add("l2norm 2e18 backward", "D16", g, gw, gA, I.c_rows(16))
    w.close()
    big = one_signed((9, 1000), 2) * 2e18
    ref = F_.normalize(big, dim=-1)
    assert int(torch.count_nonzero(ref)) == 0                              # torch float32 on the CPU: norm = inf, y = 0
    bigr = big.clone().requires_grad_(True)
    dy = one_signed((9, 1000), 3)
    F_.normalize(bigr, dim=-1).backward(dy)
    assert int(torch.count_nonzero(bigr.grad)) == 0                        # ... and its gradient is 0, not nan
    bc = big.cuda().requires_grad_(True)
    y = ops.l2_normalize(bc)
    y.backward(dy.cuda())
    torch.cuda.synchronize()
    assert torch.equal(y.detach().cpu(), ref)
    assert torch.equal(bc.grad.cpu(), bigr.grad)                           # inv = 1 / inf = 0, unclamped: dx = 0 (dy - y <y, dy>) = 0


# ---- pair_dot -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", ROW_DIMS)
def test_pair_dot_against_float64(D):
    from recbox_amd import ops
    w = Worst()
    label = "pairdot<%d>" % I.lane_group(D)
    for kind in ("randn", "one_signed", "spread"):
        for N, B, u3, needs in ((1, 257, False, (True, True)), (5, 61, True, (True, True)), (101, 7, False, (True, True)),
                                (5, 61, False, (True, False)), (5, 61, True, (False, True))):
            u = KINDS[kind]((B, 1, D) if u3 else (B, D), D + N)
            v = KINDS[kind]((B, N, D) if N > 1 else (B, D), D + N + 1)
            g = KINDS[kind]((B, N), 5)
            uc, vc = u.cuda().requires_grad_(needs[0]), v.cuda().requires_grad_(needs[1])
            out = ops.pair_dot(uc, vc, 0.37)
            out.backward(g.cuda())
            torch.cuda.synchronize()
            t = "D%d N%d %s needs=%s" % (D, N, kind, needs)
            w.add(label + " forward", t, out, *I.pair_dot64(u, v, 0.37), I.c_rows(D))
            (du, a_du), (dv, a_dv) = I.pair_dot_grad64(u, v, g, 0.37)
            if needs[0]:
                w.add(label + " du", t, uc.grad, du, a_du, I.c_rows(D))
            else:
                assert uc.grad is None
            if needs[1]:
                w.add(label + " dv", t, vc.grad, dv, a_dv, I.c_rows(D))
            else:
                assert vc.grad is None
    w.close()


def test_pair_dot_past_the_grid_cap():
    from recbox_amd import ops
    w = Worst()
    for D, B, N in ((64, 83, 101), (1, 2048 * 256 + 5, 1), (64, 2048 * 4 + 37, 2)):
        u, v, g = randn((B, D), 1), randn((B, N, D), 2), randn((B, N), 3)
        uc, vc = u.cuda().requires_grad_(True), v.cuda().requires_grad_(True)
        out = ops.pair_dot(uc, vc, 1.0)
        out.backward(g.cuda())
        torch.cuda.synchronize()
        label, t = "pairdot<%d> past the cap" % I.lane_group(D), "D%d B%d N%d" % (D, B, N)
        w.add(label + " forward", t, out, *I.pair_dot64(u, v), I.c_rows(D))
        (du, a_du), (dv, a_dv) = I.pair_dot_grad64(u, v, g)
        w.add(label + " du", t, uc.grad, du, a_du, I.c_rows(D))
        w.add(label + " dv", t, vc.grad, dv, a_dv, I.c_rows(D))
    w.close()


# ---- pool -----------------------------------------------------------------------------------------------------------------------
def _pool_inputs(B, L, D, seed, kind=randn):
    e = value_safe(kind((B, L, D), seed))
    gen = torch.Generator().manual_seed(seed + 1)
    mask = (torch.rand(B, L, generator=gen) < 0.6).float()
    if B > 2:
        e[1] = 0                                                            # an all-zero sample: value count 0
        e[2, L // 2:] = 0                                                   # trailing padding rows
        mask[0] = 0                                                         # an empty mask: denominator 0 + eps
    return e, mask


@pytest.mark.parametrize("D", ROW_DIMS)
def test_pool_against_float64(D):
    from recbox_amd import ops
    w = Worst()
    label = "pool<%d>" % I.lane_group(D)
    for L in (1, 3, 50, 300):
        B = 61 if L * D <= 20000 else 7
        for kind in (("randn", "one_signed", "spread") if L in (3, 300) else ("randn",)):
            e, mask = _pool_inputs(B, L, D, D + L, KINDS[kind])
            dout = KINDS[kind]((B, D), 7)
            for denom in (0, 1, 2, 3):
                for numer_masked in (False, True):
                    ec = e.cuda().requires_grad_(True)
                    out = ops.pool(ec, mask.cuda(), numer_masked, denom, 1e-12)
                    out.backward(dout.cuda())
                    torch.cuda.synchronize()
                    t = "D%d L%d %s denom%d masked=%s" % (D, L, kind, denom, numer_masked)
                    w.add(label + " forward", t, out, *I.pool64(e, mask, numer_masked, denom, 1e-12), I.c_pool(L))
                    w.add(label + " backward", t, ec.grad, *I.pool_grad64(e, dout, mask, numer_masked, denom, 1e-12), I.C_BOUND)
    w.close()


def test_pool_past_the_grid_cap():
    from recbox_amd import ops
    w = Worst()
    for D, B, L in ((64, 2048 * 4 + 37, 3), (1, 2048 * 256 + 5, 2), (200, 2048 * 4 + 37, 2)):
        e, mask = _pool_inputs(B, L, D, D)
        dout = randn((B, D), 1)
        ec = e.cuda().requires_grad_(True)
        out = ops.pool(ec, mask.cuda(), True, 1, 1e-12)
        out.backward(dout.cuda())
        torch.cuda.synchronize()
        label, t = "pool<%d> past the cap" % I.lane_group(D), "D%d B%d" % (D, B)
        w.add(label + " forward", t, out, *I.pool64(e, mask, True, 1, 1e-12), I.c_pool(L))
        w.add(label + " backward", t, ec.grad, *I.pool_grad64(e, dout, mask, True, 1, 1e-12), I.C_BOUND)
    w.close()


@pytest.mark.parametrize("D", [1, 16, 100, 200])
def test_every_pooling_module_against_float64(D):
    """MaskedAveragePooling / MaskedSumPooling (ranking and core), rechub AveragePooling / SumPooling with and without a
    mask, and interaction_rowsum's [B, F, 1]."""
    from recbox_amd import ops
    from recbox_amd.core.pytorch.layers import sequence as core
    from recbox_amd.ranking.pytorch.layers import pooling as rank
    from recbox_amd.rechub.basic import layers as hub
    w = Worst()
    B, L = 61, 50
    e, mask = _pool_inputs(B, L, D, D)
    mc = mask.cuda()
    e16 = float(torch.tensor(1e-16))
    cases = [("ranking MaskedAveragePooling", lambda x: rank.MaskedAveragePooling()(x), (None, False, 1, 1e-12)),
             ("ranking MaskedAveragePooling mask", lambda x: rank.MaskedAveragePooling()(x, mc), (mask, False, 2, 1e-12)),
             ("ranking MaskedSumPooling", lambda x: rank.MaskedSumPooling()(x), (None, False, 0, 0.0)),
             ("core MaskedAveragePooling", lambda x: core.MaskedAveragePooling()(x), (None, False, 1, 1e-12)),
             ("core MaskedSumPooling", lambda x: core.MaskedSumPooling()(x), (None, False, 0, 0.0)),
             ("rechub AveragePooling", lambda x: hub.AveragePooling()(x), (None, False, 3, 0.0)),
             ("rechub AveragePooling mask", lambda x: hub.AveragePooling()(x, mc), (mask, True, 2, e16)),
             ("rechub SumPooling", lambda x: hub.SumPooling()(x), (None, False, 0, 0.0)),
             ("rechub SumPooling mask", lambda x: hub.SumPooling()(x, mc), (mask, True, 0, 0.0))]
    dout = randn((B, D), 3)
    for name, run, (m, nm, denom, eps) in cases:
        ec = e.cuda().requires_grad_(True)
        out = run(ec)
        out.backward(dout.cuda())
        torch.cuda.synchronize()
        w.add("pool modules forward", "%s D%d" % (name, D), out, *I.pool64(e, m, nm, denom, eps), I.c_pool(L))
        w.add("pool modules backward", "%s D%d" % (name, D), ec.grad, *I.pool_grad64(e, dout, m, nm, denom, eps), I.C_BOUND)
    col = randn((B, 39, 1), 4)
    cc = col.cuda().requires_grad_(True)
    out = ops.interaction_rowsum(cc)
    out.backward(dout[:, :1].cuda())
    torch.cuda.synchronize()
    w.add("pool modules forward", "interaction_rowsum", out, *I.pool64(col), I.c_pool(39))
    w.add("pool modules backward", "interaction_rowsum", cc.grad, *I.pool_grad64(col, dout[:, :1]), I.C_BOUND)
    w.close()


# ---- determinism ----------------------------------------------------------------------------------------------------------------
def test_every_op_twice_gives_the_same_bits_and_backward_twice_over_one_forward():
    from recbox_amd import ops
    B, F, D = 257, 39, 100
    e, g3 = randn((B, F, D), 1).cuda(), randn((B, F * (F - 1) // 2, D), 2).cuda()
    mask = (torch.rand(B, F, device="cuda") < 0.5).float()
    u = randn((B, D), 3).cuda()
    runs = {
        "product_sum": (lambda x: ops.interaction(x, "product_sum"), e),
        "bi_interaction": (lambda x: ops.interaction(x, "bi_interaction"), e),
        "inner_product": (lambda x: ops.interaction(x, "inner_product"), e),
        "elementwise_product": (lambda x: ops.interaction(x, "elementwise_product"), e),
        "pair_mul": (lambda x: ops.pair_mul(x, e, False), e),
        "pair_mul per pair": (lambda x: ops.pair_mul(x, e, True), g3),
        "l2_normalize": (lambda x: ops.l2_normalize(x), e),
        "pair_dot": (lambda x: ops.pair_dot(u, x, 0.5), e),
        "pool": (lambda x: ops.pool(x, mask, True, 1, 1e-12), e),
    }
    lin1, lr = torch.nn.Linear(F * D + 4, 32).cuda(), torch.nn.Linear(F * D, 1).cuda()
    block = torch.cat([e.reshape(B, -1), randn((B, 4), 4).cuda()], 1)

    def stage(x):                                                         # the three outputs as one tensor: one backward drives all
        lin1.zero_grad()
        lr.zero_grad()
        h, y_fm, y_lr = ops.deepfm_input_stage(x, lin1, lr, F * D, D)
        return torch.cat([h, y_fm, y_lr], 1)

    assert ops.deepfm_input_stage_supported(block, F * D, D)
    runs["deepfm_input_stage"] = (stage, block)
    for name, (fn, x) in runs.items():
        outs, grads = [], []
        for _ in range(2):
            xc = x.clone().requires_grad_(True)
            out = fn(xc)
            r = torch.ones_like(out) * 0.75
            out.backward(r, retain_graph=True)
            first = xc.grad.clone()
            xc.grad = None
            out.backward(r)                                               # the same forward, a second backward
            torch.cuda.synchronize()
            assert torch.equal(xc.grad, first), name + ": backward twice over one forward differs"
            outs.append(out.detach())
            grads.append(first)
        assert torch.equal(outs[0], outs[1]), name + ": forward differs between two runs"
        assert torch.equal(grads[0], grads[1]), name + ": backward differs between two runs"
