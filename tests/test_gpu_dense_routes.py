"""One small case per route of the dense GEMM family (recbox_amd/csrc/rbx_dense.hip: the try_* functions of run_gemm and
rbx_linear_bwd; DESIGN.md lists them in priority order), each against a float64 product computed with torch on the CPU.

Shapes are the smallest that select the route and still reach its edge handling.  f32 routes: randn inputs with one operand
divided by sqrt(red) and the tolerance 2e-5 * max(1, sqrt(red) / 8), red the reduction length (as test_gpu_matching.py).
Split-operand routes: the rule of test_split_bf16_gemm_runs_and_is_as_accurate_as_the_f32_mfma -- the error e6 against
float64 is at most max(4 e32, 2e-6 scale) and at most 1e-5 scale, e32 the error of the same product on the f32 MFMAs -- and
rbx_gemm_bx6_count moves by exactly the number of split-operand launches (by zero on the f32 routes).

Margins of the bounds for these seeds, from torch's f32 matmul on the CPU against the float64 references: the f32 formula
holds 12-23 times over on the forward / dx / slab cases (errors 0.9-2.3e-6) and 100-650 times over on the weight gradients
(1.2-1.7e-6 against 1.6-2.3e-4); 1e-5 * scale holds 15-32 times over on the split-operand cases (0.8-2.2e-7)."""
import pytest
import torch

from conftest import assert_close

pytestmark = pytest.mark.gpu


def f32_tol(red):
    return 2e-5 * max(1.0, red ** 0.5 / 8)


def _gen(*key):
    return torch.Generator().manual_seed(sum(key))


class _split_launches:
    """the launch counter of the split-operand kernels moves by exactly `expect` inside the block"""

    def __init__(self, expect=0):
        self.expect = expect

    def __enter__(self):
        from recbox_amd import ops
        self.n0 = ops.gemm_bx6_count()

    def __exit__(self, *exc):
        from recbox_amd import ops
        if exc[0] is None:
            assert ops.gemm_bx6_count() == self.n0 + self.expect


def _assert_split_accuracy(name, got6, got32, want):
    e6 = float((got6.double().cpu() - want).abs().max())
    e32 = float((got32.double().cpu() - want).abs().max())
    scale = float(want.abs().max())
    print("%s: e6 %.3e e32 %.3e scale %.3e" % (name, e6, e32, scale))
    assert e6 <= max(4.0 * e32, 2e-6 * scale), (name, e6, e32, scale)
    assert e6 <= 1e-5 * scale, (name, e6, scale)


# ---- the f32 tile kernel -------------------------------------------------------------------------------------------------------
# M = 160: one full row tile plus an edge with one 32-block (the dealt placement).  Output columns 144 / 176: a tail of 16 / 48
# behind a full column tile, the narrow tile with NT = 1 / 2 inside the main launch; 100: the narrow kernel alone.
# Reduction 49: unaligned rows, one steady iteration, a guarded last tile; 64: aligned.
@pytest.mark.parametrize("red", [49, 64])
@pytest.mark.parametrize("out", [144, 176, 100])
def test_f32_tile_kernel_forward_and_dx(out, red):
    from recbox_amd import ops
    M = 160
    g = _gen(M, out, red)
    x = torch.randn(M, red, generator=g)
    w = torch.randn(out, red, generator=g) / red ** 0.5
    b = torch.randn(out, generator=g)
    wt = torch.randn(red, out, generator=g) / red ** 0.5                      # dx = dy W: W [red, out]
    with _split_launches():
        y = ops._lin_fwd(x.cuda(), w.cuda(), b.cuda())
        dx = ops._lin_dx(x.cuda(), wt.cuda())
    assert_close(y, (x.double() @ w.double().t() + b.double()), f32_tol(red), "y")
    assert_close(dx, (x.double() @ wt.double()), f32_tol(red), "dx")


def _dwdb(x, dy):
    from recbox_amd import ops
    n, k = dy.shape[1], x.shape[1]
    w = torch.zeros(n, k, device="cuda")
    dw = torch.empty(n, k, device="cuda")
    db = torch.empty(n, device="cuda")
    ops._lin_dwdb(x.cuda(), w, dy.cuda(), dw, db)
    return dw, db


def _dw_inputs(m, n, k):
    g = _gen(m, n, k)
    x = torch.randn(m, k, generator=g)
    dy = torch.randn(m, n, generator=g) / m ** 0.5
    return x, dy


def test_f32_split_k_and_fixed_order_reduce():
    """m = 4096 is below the bxt threshold of 8192: dW [130, 130] is split along K on the f32 kernel and reduced"""
    m, n, k = 4096, 130, 130
    x, dy = _dw_inputs(m, n, k)
    with _split_launches():
        dw, db = _dwdb(x, dy)
    assert_close(dw, (dy.double().t() @ x.double()), f32_tol(m), "dw")
    assert_close(db, dy.double().sum(0), f32_tol(m), "db")


# ---- bxt: the weight gradient on the split-operand kernel with transposed staging ----------------------------------------------
def test_bxt_weight_gradient():
    """m = 8192 + 24, dW [200, 144]: one 256-row tile that is more than 3/4 full, with an edge column tile.  e32: the same
    product on the f32 tile kernel, as a dx GEMM of the transposed gradient (no split-K, another summation order): the
    library reads RBX_GEMM_BX6 once per process, so the same rbx_linear_bwd call cannot run with the splitting off here."""
    from recbox_amd import ops
    m, n, k = 8192 + 24, 200, 144
    g = _gen(m, n, k)
    x = torch.rand(m, k, generator=g)
    dy = torch.rand(m, n, generator=g) / m
    want = dy.double().t() @ x.double()
    with _split_launches(1):
        dw6, db = _dwdb(x, dy)
    with _split_launches():
        dw32 = ops._lin_dx(dy.t().contiguous().cuda(), x.cuda())
    _assert_split_accuracy("dw", dw6, dw32, want)
    assert_close(db, dy.double().sum(0), f32_tol(m), "db")


def test_bxt_tile_less_than_three_quarters_full_stays_on_f32():
    """dW [128, 144]: the 256-row tile would be half empty, so the f32 split-K route takes it and the counter stays"""
    m, n, k = 8192 + 24, 128, 144
    x, dy = _dw_inputs(m, n, k)
    with _split_launches():
        dw, db = _dwdb(x, dy)
    assert_close(dw, (dy.double().t() @ x.double()), f32_tol(m), "dw")
    assert_close(db, dy.double().sum(0), f32_tol(m), "db")


# ---- the streaming kernels of [M, 64 / 128] activations ------------------------------------------------------------------------
@pytest.mark.parametrize("M,K,N,fused", [(2048 + 5, 64, 64, False), (2048 + 5, 64, 64, True),
                                         (2080, 64, 128, False), (2080, 64, 128, True),
                                         (2080, 128, 64, False), (2080, 128, 64, True)])
def test_k64n64_and_slab_kernels(M, K, N, fused):
    """64 -> 64 (weights in registers; fused: residual plus row scale) and 64 -> 128 / 128 -> 64 (weights in LDS; fused:
    residual), with a last slab of 5 / 32 rows"""
    from recbox_amd import ops
    g = _gen(M, K, N)
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    b = torch.randn(N, generator=g)
    res = torch.randn(M, N, generator=g) if fused else None
    rs = (torch.rand(M, generator=g) > 0.3).float() * 1.5 if fused and N == 64 and K == 64 else None
    want = x.double() @ w.double().t() + b.double()
    if res is not None:
        want = want + res.double()
    if rs is not None:
        want = want * rs.double()[:, None]
    with _split_launches():
        y = ops._lin_fwd(x.cuda(), w.cuda(), b.cuda(), residual=res.cuda() if fused else None,
                         row_scale=rs.cuda() if rs is not None else None)
    assert_close(y, want, f32_tol(K), "y")


# ---- registered planes, through the C ABI (ops registers planes only from M = 4096 on) -----------------------------------------
def _planes_call(x, w, transposed, register):
    """y = x W^T (transposed = 0, W [out, red]) or dx = x W (transposed = 1, W [red, out]) with W's planes registered or not"""
    from recbox_amd import ops
    lib, ptr = ops.lib, ops._ptr
    M = x.shape[0]
    rows, cols = w.shape
    out = cols if transposed else rows
    y = torch.empty(M, out, device="cuda")
    planes = torch.empty(lib.rbx_split_bf16_size(rows, cols, transposed), dtype=torch.uint8, device="cuda")
    if register:
        ops.check(lib.rbx_split_bf16(ptr(w), cols, rows, cols, transposed, ptr(planes), ops._stream()))
        ops.check(lib.rbx_split_register(ptr(w), ptr(planes), rows, cols, transposed))
    try:
        if transposed:
            ops.check(lib.rbx_linear_dx_fused(ptr(x), x.stride(0), ptr(w), M, rows, cols, None, cols, None, cols, ptr(y), cols,
                                              ops._stream()))
        else:
            ops.check(lib.rbx_linear_fwd(ptr(x), x.stride(0), ptr(w), None, M, rows, cols, 0, ptr(y), ops._stream()))
    finally:
        if register:
            lib.rbx_split_unregister(ptr(w))
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize("transposed", [0, 1])
@pytest.mark.parametrize("M,out,red", [(160, 144, 72),         # M < 512: gemm_bx6_kernel, dealt edge tiles
                                       (552, 144, 200)])       # gemm_bxp_kernel: steady loop entered, edge tiles both ways
def test_registered_planes(M, out, red, transposed):
    g = _gen(M, out, red, transposed)
    x = torch.rand(M, red, generator=g)                        # one-signed, like ReLU outputs
    w = torch.rand(*((red, out) if transposed else (out, red)), generator=g) / red
    want = x.double() @ (w.double() if transposed else w.double().t())
    xc, wc = x.cuda(), w.cuda()
    with _split_launches():
        y32 = _planes_call(xc, wc, transposed, register=False)
    with _split_launches(1):
        y6 = _planes_call(xc, wc, transposed, register=True)
    _assert_split_accuracy("y", y6, y32, want)


# ---- n == 1: the logit head ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [50, 52])                        # rows that are not / are 16-byte aligned: scalar / vector path
def test_logit_head_forward_and_backward(k):
    from recbox_amd import ops
    m = 1030
    g = _gen(m, k)
    x = torch.randn(m, k, generator=g)
    w = torch.randn(1, k, generator=g) / k ** 0.5
    b = torch.randn(1, generator=g)
    R = torch.randn(m, 1, generator=g) / m ** 0.5
    xc, wc, bc = (t.clone().cuda().requires_grad_(True) for t in (x, w, b))
    with _split_launches():
        y = ops.linear(xc, wc, bc, None)
        (y * R.cuda()).sum().backward()
    assert_close(y, (x.double() @ w.double().t() + b.double()), f32_tol(k), "y")
    assert_close(xc.grad, (R.double() @ w.double()), f32_tol(1), "dx")
    assert_close(wc.grad, (R.double().t() @ x.double()), f32_tol(m), "dw")
    assert_close(bc.grad, R.double().sum(0), f32_tol(m), "db")


# ---- tall and narrow weight gradients ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,k", [(8192 + 3, 70, 33),         # tall_dw_kernel<2>, ragged quadrants, a ragged last row pair
                                   (8192 + 3, 64, 64),         # the slab form, a last slab of 3 rows
                                   (8192, 128, 64)])           # the slab form once per 64-column half of g
def test_tall_weight_gradients(m, n, k):
    x, dy = _dw_inputs(m, n, k)
    with _split_launches():
        dw, db = _dwdb(x, dy)
    assert_close(dw, (dy.double().t() @ x.double()), f32_tol(m), "dw")
    assert_close(db, dy.double().sum(0), f32_tol(m), "db")


def test_tall_weight_gradient_with_scaled_rows():
    from recbox_amd import ops
    m = 8192
    x, dy = _dw_inputs(m, 64, 64)
    rs = (torch.rand(m, generator=_gen(m)) > 0.3).float() * 1.5
    dw = torch.empty(64, 64, device="cuda")
    db = torch.empty(64, device="cuda")
    with _split_launches():
        ops._lin_dwdb_scaled(x.cuda(), dy.cuda(), rs.cuda(), dw, db)
    sdy = dy.double() * rs.double()[:, None]
    assert_close(dw, (sdy.t() @ x.double()), f32_tol(m), "dw")
    assert_close(db, sdy.sum(0), f32_tol(m), "db")
