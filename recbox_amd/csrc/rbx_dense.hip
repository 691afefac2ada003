// rbx_dense.hip -- dense tower contractions on the fp32 matrix cores (gfx950).
//
// Reference behaviour replaced: every nn.Linear of the MLP towers
//   core/pytorch/layers/mlp.py:25-37, ranking/pytorch/layers/blocks/mlp_block.py:42-58,
//   third_party/rechub/basic/layers.py:255-263 (and the 1x1-conv FFN / attention
//   projections of third_party/rechub/models/matching/sasrec.py:81-94,110-124)
// forward  y  = act(x W^T + b)          x[M,K] W[N,K]
// backward dx = dy' W,  dW = dy'^T x,  db = colsum(dy'),  dy' = dy * act'(y)
//
// BASELINE.json asks for fp32 logits within 1e-4, and CDNA4 has no TF32: the kernels use
// v_mfma_f32_32x32x2_f32 (exact fp32 products and accumulation, 256 FLOP/clk/CU) rather
// than bf16 MFMA.  One GEMM kernel serves the three contractions through operand layout
// flags.  Tile 128x128x16 per 256-thread workgroup, 2x2 waves, each wave 2x2 MFMA tiles
// of 32x32 (64 accumulator VGPRs).  Operands are staged k-major in LDS (As[k][m],
// Bs[k][n]) so an MFMA operand read is 32 consecutive floats per half-wave: conflict
// free.  Steady state of the k loop (gemm_steady): the next tile's global loads are issued
// first (inline assembly, no tests), parked in the other LDS buffer halfway through the
// current tile's 32 MFMAs, one barrier per k tile, four wavefronts per SIMD; the last two
// k tiles run the tested loop.  Tiles on the matrix edge take the same loop, skip the
// 32 x 32 blocks that hold no output and share the live ones between their wavefronts; a
// narrow tail of output columns rides in the same launch (narrow_tile).  The
// weight-gradient GEMM has a tiny output and K = batch, so it is split along K across
// workgroups (one flat launch, full tiles first) into a workspace and reduced in a fixed
// order (deterministic, no float atomics).  What was measured on the way:
// profiles/r02/gemm_variants.txt.
//
// The kernels: rbx_gemm_tile.h (what the tiled kernels share), rbx_gemm_f32.h, rbx_gemm_bx.h (split operands on the bf16
// MFMAs), rbx_gemm_slab.h (everything else).  This file is the host side: every route is a function whose first lines are
// its condition; run_gemm and rbx_linear_bwd try them in priority order (DESIGN.md lists them).
#include <stdlib.h>
#include <atomic>
#include <mutex>
#include <type_traits>
#include "rbx_internal.h"
#include "rbx_gemm_tile.h"
#include "rbx_gemm_f32.h"
#include "rbx_gemm_bx.h"
#include "rbx_gemm_slab.h"

namespace rbx {

static bool vec_ok(const float* p, long long ld) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && (ld % 4) == 0; }

// RBX_GEMM_BX6=0: every GEMM on v_mfma_f32_32x32x2_f32 (exact f32 products; A/B measurements, debugging); default: weights
// with registered bf16 planes, and the weight gradient of a large batch, run the split-operand kernels on the bf16 matrix cores
static bool bx6_mode() {
  static const bool v = [] { const char* e = getenv("RBX_GEMM_BX6"); return !(e != nullptr && atoi(e) == 0); }();
  return v;
}
// weights whose bf16 planes the caller has made for the GEMM calls it is about to issue (rbx_split_register)
struct SplitEntry {
  const float* w;
  const unsigned short* planes;
  int rows, cols, transposed;
};
constexpr int kSplitSlots = 256;   // registrations live for the duration of ONE call (a tower layer); 256 concurrent ones (threads x towers) before a GEMM falls back to the f32 kernel
static SplitEntry g_split[kSplitSlots];
static std::mutex g_split_mu;
static std::atomic<unsigned long long> g_bx6_launches{0};     // observability: GEMMs that ran on the split-operand kernel
static bool split_find(const float* w, int transposed, int rows, int cols, SplitEntry* out) {
  std::lock_guard<std::mutex> lock(g_split_mu);
  for (int i = 0; i < kSplitSlots; ++i)
    if (g_split[i].w == w && g_split[i].planes != nullptr && g_split[i].transposed == transposed && g_split[i].rows == rows &&
        g_split[i].cols == cols) {
      *out = g_split[i];
      return true;
    }
  return false;
}

static void launch_splitk_reduce(hipStream_t s, unsigned blocks, const float* part, long long n, int splits, float* out,
                                 const float* part2 = nullptr, long long n2 = 0, float* out2 = nullptr) {
  const unsigned blocks2 = part2 != nullptr ? static_cast<unsigned>((n2 + 63) / 64) : 0u;
  hipLaunchKernelGGL(splitk_reduce_kernel, dim3(blocks + blocks2), dim3(64 * kRedZ), 0, s, part, n, splits, out, part2, n2,
                     out2, static_cast<int>(blocks));
}
// blocks of outer_kernel: a multiple of the row length in vectors where that fits, so that a lane keeps its columns
static unsigned outer_grid(long long total_vecs, long long per_row) {
  long long blocks = (total_vecs + 255) / 256;
  const long long cap = kCUs * 16;
  if (blocks > cap) blocks = cap;
  long long a = per_row, b = 256;
  while (b != 0) { const long long t = a % b; a = b; b = t; }
  const long long unit = per_row / a;
  if (unit <= blocks) blocks = blocks / unit * unit;
  return static_cast<unsigned>(blocks < 1 ? 1 : blocks);
}
// grid of an element-wise or reduce kernel: one block per `per_block` items, at most 8 per CU
static unsigned capped_grid(long long items, int per_block) {
  long long blocks = (items + per_block - 1) / per_block;
  if (blocks > kCUs * 8) blocks = kCUs * 8;
  return static_cast<unsigned>(blocks);
}
// out[n] = the fixed-order sum of `splits` partials of n floats each
static int reduce_partials(hipStream_t s, const float* part, long long n, int splits, float* out) {
  launch_splitk_reduce(s, capped_grid(n, 64), part, n, splits, out);
  return check_launch("splitk_reduce_kernel");
}
// workgroups of a slab kernel over M rows: a wavefront per 32-row slab, at most two workgroups of four wavefronts per CU
// (two wavefronts per SIMD)
static int slab_grid(int M) {
  const int slabs = (M + 31) / 32;
  const int wgs = (slabs + kSlabWaves - 1) / kSlabWaves;
  return wgs > 2 * kCUs ? 2 * kCUs : wgs;
}

// C[M, N] (ldc) = epilogue(act(op(A) op(B) + bias)); AK / BK_ (template arguments of the routes): the operand is
// k-contiguous.  ws: split-K scratch of ws_floats floats, or NULL.  bias, act, ws and epi are set by name where a call has them.
struct GemmCall {
  const float *A; long long lda;
  const float *B; long long ldb;
  float* C; long long ldc;
  int M, N, K;
  hipStream_t s;
  const float* bias = nullptr;
  int act = 0;
  float* ws = nullptr; size_t ws_floats = 0;
  Epi epi = Epi{};
  bool has_epi() const { return epi.res != nullptr || epi.mask != nullptr || epi.rowscale != nullptr || epi.fm_x != nullptr; }
  int tiles_m() const { return (M + BM - 1) / BM; }
  int tiles_n() const { return (N + BN - 1) / BN; }
};

// K slices of the f32 tile kernel (1: no split)
static int plan_splitk(const GemmCall& c) {
  const long long tiles = static_cast<long long>(c.tiles_m()) * c.tiles_n();
  // tiny output, long reduction: split K
  if (!(tiles < kCUs && c.K >= 4096 && c.ws != nullptr && c.ldc == c.N && !c.has_epi())) return 1;
  // every workgroup of the launch is resident at once (33.8 KB of LDS each), so the kernel lasts as long as the CU
  // with the most workgroups: pick the split count whose tiles x splits fills whole rounds of the 256 CUs best
  // (k = 1677: 56 tiles x 10 splits = 560 workgroups left a third of the chip idle during the last round; x 9 = 504 fits)
  // Sized on the tiles with 128 x 128 real outputs: the edge tiles are launched after them and cost a fraction
  // (M = 400 is three full rows of tiles and one with 16 rows -- counted as full, the 56 tiles of cfg 4's layer-1 dW
  // got 9 slices (455 k steps each) where the 42 full ones fill the chip with 12 (341 steps)).
  const long long n_full = static_cast<long long>(c.M / BM) * (c.N / BN);
  const long long sized = n_full > 0 ? n_full : tiles;
  // (slices of at least 512 reduction rows; a SHORT reduction -- K < 32 768: the weight gradient of a tower at the per-GPU
  //  batch of an 8-GPU strong-scaling run -- may be cut into slices of 128, or its handful of workgroups walk the whole
  //  batch on a few CUs: [128, 256] x 8 192 rows took 54 us in 32 workgroups, profiles/r06/small_batches.txt)
  const int max_splits = c.K >= 32768 ? c.K / 512 : c.K / 128;
  const long long fit = static_cast<long long>(c.ws_floats / (static_cast<size_t>(c.M) * c.N));
  int best = 1;
  double best_eff = 0.0;
  for (int sp = 1; sp <= max_splits && sp <= fit && tiles * sp <= 4 * kCUs; ++sp) {
    const long long wgs = sized * sp;
    const long long rounds = (wgs + kCUs - 1) / kCUs;
    double eff = static_cast<double>(wgs) / static_cast<double>(rounds * kCUs);
    if (rounds < 2) eff *= 0.9;                      // one workgroup per CU hides less latency than two
    if (eff > best_eff + 1e-9) { best_eff = eff; best = sp; }
  }
  return best;
}

// Each try_* returns whether it took the call, with the call's status in *rc.
// 64 -> 64 over many rows: the streaming kernel with the weights in registers
template <bool AK, bool BK_>
static bool try_k64n64(const GemmCall& c, int splits, int* rc) {
  if (!(AK && c.K == 64 && c.N == 64 && splits == 1 && c.epi.fm_x == nullptr && c.M >= 2048 && vec_ok(c.A, c.lda) &&
        (!BK_ || vec_ok(c.B, c.ldb))))
    return false;
  const dim3 grid(slab_grid(c.M)), block(64 * kSlabWaves);
  const int code = (c.epi.res != nullptr ? 1 : 0) | (c.epi.mask != nullptr ? 2 : 0) | (c.epi.rowscale != nullptr ? 4 : 0) | (c.act == 1 ? 8 : 0);
#define RBX_K64(E) case E: hipLaunchKernelGGL((gemm_f32_k64n64_kernel<BK_, E>), grid, block, 0, c.s, c.A, c.lda, c.B, c.ldb, c.C, c.ldc, c.M, c.bias, c.epi); break
  switch (code) {
    RBX_K64(0); RBX_K64(1); RBX_K64(2); RBX_K64(3); RBX_K64(4); RBX_K64(5); RBX_K64(6); RBX_K64(7);
    RBX_K64(8); RBX_K64(9); RBX_K64(10); RBX_K64(11); RBX_K64(12); RBX_K64(13); RBX_K64(14); RBX_K64(15);
  }
#undef RBX_K64
  *rc = check_launch("gemm_f32_k64n64_kernel");
  return true;
}

// dW = dy^T x of a compute-bound tower layer: the split-operand kernel with transposed staging, K (the batch) split
template <bool AK, bool BK_>
static bool try_bxt_dw(const GemmCall& c, int* rc) {
  if (!(!AK && !BK_ && bx6_mode() && c.ws != nullptr && !c.has_epi() && c.ldc == c.N && c.K >= 8192 && c.M >= 128 &&
        c.N >= 128))
    return false;
  const int M = c.M, N = c.N, K = c.K;
  const int tm2 = (M + PBM - 1) / PBM;
  const int n_tiles = tm2 * c.tiles_n();
  int sp = kCUs / n_tiles;                           // one workgroup per CU (108 KB of LDS each): one round of the chip
  if (4 * M < 3 * tm2 * PBM) sp = 0;                 // 256-row tiles less than 3/4 full (M = 128): the f32 kernel's 128-row tiles
  const long long fit = static_cast<long long>(c.ws_floats / (static_cast<size_t>(M) * N));
  if (sp > fit) sp = static_cast<int>(fit);
  if (sp > K / (K >= 32768 ? 1024 : 256)) sp = K / (K >= 32768 ? 1024 : 256);      // (short reductions: see plan_splitk)
  if (sp < 1) return false;
  int kps = (K + sp - 1) / sp;
  kps = (kps + PBK - 1) / PBK * PBK;
  sp = (K + kps - 1) / kps;
  static bool attr_set = false;
  if (!attr_set) {
    if ((*rc = allow_lds("gemm_bxt_kernel", gemm_bxt_kernel, kBxPipeLds)) != RBX_OK) return true;
    attr_set = true;
  }
  hipLaunchKernelGGL(gemm_bxt_kernel, dim3(n_tiles * sp), dim3(PTHREADS), kBxPipeLds, c.s, c.A, c.lda, c.B, c.ldb, c.ws, M, N, K,
                     kps, c.tiles_n(), n_tiles);
  *rc = check_launch("gemm_bxt_kernel");
  if (*rc != RBX_OK) return true;
  g_bx6_launches.fetch_add(1, std::memory_order_relaxed);
  *rc = reduce_partials(c.s, c.ws, static_cast<long long>(M) * N, sp, c.C);
  return true;
}

// 64 -> 128 and 128 -> 64 over many rows: the slab kernel with the weights in LDS
template <bool AK, bool BK_>
static bool try_slabw(const GemmCall& c, int splits, int* rc) {
  if (!(AK && splits == 1 && c.epi.fm_x == nullptr && c.epi.mask == nullptr && c.epi.rowscale == nullptr && c.M >= 2048 &&
        vec_ok(c.A, c.lda) && ((c.K == 64 && c.N == 128) || (c.K == 128 && c.N == 64))))
    return false;
  const dim3 grid(slab_grid(c.M)), block(64 * kSlabWaves);
#define RBX_SLABW(KH_, NT_, R) hipLaunchKernelGGL((gemm_f32_slabw_kernel<KH_, NT_, BK_, R>), grid, block, 0, c.s, c.A, c.lda, c.B, c.ldb, c.C, c.ldc, c.M, c.bias, c.act, c.epi)
  if (c.K == 64) { if (c.epi.res != nullptr) RBX_SLABW(1, 4, true); else RBX_SLABW(1, 4, false); }
  else { if (c.epi.res != nullptr) RBX_SLABW(2, 2, true); else RBX_SLABW(2, 2, false); }
#undef RBX_SLABW
  *rc = check_launch("gemm_f32_slabw_kernel");
  return true;
}

// weights with registered bf16 planes: the split-operand kernels on the bf16 matrix cores
template <bool AK, bool BK_>
static bool try_planes(const GemmCall& c, int splits, int* rc) {
  SplitEntry e;
  if (!(AK && splits == 1 && bx6_mode() && split_find(c.B, BK_ ? 0 : 1, BK_ ? c.N : c.K, BK_ ? c.K : c.N, &e))) return false;
  const int kp = (c.K + SBK - 1) / SBK * SBK;
  const int tn = c.tiles_n();
  const bool small = c.M < 2 * PBM;                  // few rows: the 128 x 128 form
  if (small) {
    const int tm = c.tiles_m();
    hipLaunchKernelGGL(gemm_bx6_kernel, dim3(tn * tm), dim3(256), 0, c.s, c.A, c.lda, e.planes, kp, c.C, c.ldc, c.M, c.N, c.K,
                       c.bias, c.act, tm, tn, c.epi);
  } else {
    static bool attr_set = false;
    if (!attr_set) {
      if ((*rc = allow_lds("gemm_bxp_kernel", gemm_bxp_kernel, kBxPipeLds)) != RBX_OK) return true;
      attr_set = true;
    }
    const int tm2 = (c.M + PBM - 1) / PBM;
    hipLaunchKernelGGL(gemm_bxp_kernel, dim3(tn * tm2), dim3(PTHREADS), kBxPipeLds, c.s, c.A, c.lda, e.planes, kp, c.C, c.ldc,
                       c.M, c.N, c.K, c.bias, c.act, tm2, tn, c.epi);
  }
  g_bx6_launches.fetch_add(1, std::memory_order_relaxed);
  *rc = check_launch(small ? "gemm_bx6_kernel" : "gemm_bxp_kernel");
  return true;
}

// everything else: the f32 tile kernel, with K split as planned (partials reduced in a fixed order)
template <bool AK, bool BK_>
static int run_f32(const GemmCall& c, int splits) {
  const int M = c.M, N = c.N, K = c.K, tm = c.tiles_m(), tn = c.tiles_n();
  int kps = (K + splits - 1) / splits;
  kps = (kps + BK - 1) / BK * BK;
  splits = (K + kps - 1) / kps;
  float* dst = (splits > 1) ? c.ws : c.C;
  // The last partial column tile: when it is at most 64 columns wide (and K is not split) it goes to the narrow tile, which
  // rides in the main launch when there are full column tiles in front of it (N < 128: the narrow kernel alone).  Measured
  // at cfg 4 (N = 400 = 3 x 128 + 16, profiles/r02/gemm_variants.txt): layer-1 forward 820 us with a narrow launch of its
  // own, 856 with the tail as a fourth full-width column tile (a fourth workgroup slot per row block for 4 % of the
  // columns); 400 x 400: 214 vs 230.
  const int tail = N % BN;
  const int tn_full = (splits == 1 && tail > 0 && tail <= 64) ? N / BN : tn;
  const bool inside = tn_full > 0 && tn_full < tn;       // the narrow tail rides in the main launch
  const bool vec_a = vec_ok(c.A, c.lda), vec_b = vec_ok(c.B, c.ldb);
  if (tn_full > 0)
    hipLaunchKernelGGL((gemm_f32_kernel<AK, BK_>), dim3(tn_full * tm * splits + (inside ? tm : 0)), dim3(256), 0, c.s, c.A, c.lda,
                       c.B, c.ldb, dst, (splits > 1) ? static_cast<long long>(N) : c.ldc, M, N, K, kps, c.bias, c.act, vec_a,
                       vec_b, tm, tn_full, splits, inside ? tm : 0, tail <= 32 ? 1 : 2, c.epi);
  if (tn_full < tn && !inside) {
    const int n0 = tn_full * BN;
    if (tail <= 32)
      hipLaunchKernelGGL((gemm_f32_narrow_kernel<AK, BK_, 1>), dim3(tm), dim3(256), 0, c.s, c.A, c.lda, c.B, c.ldb, c.C, c.ldc, M,
                         N, K, n0, c.bias, c.act, vec_a, vec_b, c.epi);
    else
      hipLaunchKernelGGL((gemm_f32_narrow_kernel<AK, BK_, 2>), dim3(tm), dim3(256), 0, c.s, c.A, c.lda, c.B, c.ldb, c.C, c.ldc, M,
                         N, K, n0, c.bias, c.act, vec_a, vec_b, c.epi);
  }
  const int rc = check_launch("gemm_f32_kernel");
  if (rc != RBX_OK || splits == 1) return rc;
  return reduce_partials(c.s, c.ws, static_cast<long long>(M) * N, splits, c.C);
}

// generic driver: the routes in priority order
template <bool AK, bool BK_>
static int run_gemm(const GemmCall& c) {
  const int splits = plan_splitk(c);
  int rc = RBX_OK;
  if (try_k64n64<AK, BK_>(c, splits, &rc)) return rc;
  if (try_bxt_dw<AK, BK_>(c, &rc)) return rc;
  if (try_slabw<AK, BK_>(c, splits, &rc)) return rc;
  if (try_planes<AK, BK_>(c, splits, &rc)) return rc;
  return run_f32<AK, BK_>(c, splits);
}

// y[m,n] = x[m,k] * W[n,k]^T : A = x (k contiguous), B(k,n) = W[n*k + k] (k contiguous)
static int run_fwd_gemm(const float* x, int64_t x_stride, const float* w, const float* bias, int64_t m, int32_t n, int32_t k,
                        int32_t act, float* y, int64_t y_stride, hipStream_t s, const Epi& epi) {
  GemmCall c{x, x_stride, w, k, y, y_stride, static_cast<int>(m), n, k, s};
  c.bias = bias;
  c.act = act;
  c.epi = epi;
  return run_gemm<true, true>(c);
}
// dx[m,k] = dy[m,n] * W[n,k]: A = dy (n contiguous = its K), B(kk=n, col=k) = W[n*k + k] (col contiguous)
static int run_dx_gemm(const float* dy, int64_t dy_stride, const float* w, int64_t m, int32_t n, int32_t k, float* dx,
                       int64_t dx_stride, hipStream_t s, const Epi& epi) {
  GemmCall c{dy, dy_stride, w, k, dx, dx_stride, static_cast<int>(m), k, n, s};
  c.epi = epi;
  return run_gemm<true, false>(c);
}

// split-K scratch of the weight gradient: room for 2 x CUs slices of [n, k], at most 64 MiB
// workgroups of tall_dw_kernel at most (each leaves an [n, k] partial): 4 per CU -- measured on
// SASRec's [819 200, 64] x [819 200, 64] weight gradients: 158 us with 512 workgroups, 118 with 1024, 124 with 2048 (and the
// reduce over the partials grows with them).
static int tall_wgs_max() { return 4 * kCUs; }
static size_t dw_ws_floats(int32_t n, int32_t k) {
  const size_t slices = static_cast<size_t>(tall_wgs_max() > 2 * kCUs ? tall_wgs_max() : 2 * kCUs);
  const size_t want = static_cast<size_t>(n) * k * slices;
  const size_t cap = size_t(1) << 24;
  const size_t one = static_cast<size_t>(n) * k;
  return want < cap ? want : (cap > one ? cap : one);
}

// What rbx_linear_bwd has in hand once dy' = dy * act'(y) exists: g = dy' [M, n], x [M, k] (ldx), the outputs (any of them
// may be NULL), and the workspace -- dw_floats floats of dW partials at ws, the bias partials behind them.
struct BwdCall {
  const float* g;
  const float* x; long long ldx;
  const float* w;
  int M, n, k;
  float* dx; long long lddx;
  float *dw, *db;
  float* ws; size_t dw_floats;
  hipStream_t s;
  float* db_part() const { return db != nullptr ? ws + dw_floats : nullptr; }
  bool slab_ok() const {     // the slab form of the 64-wide weight gradients: aligned rows, room for its partials
    return M >= 8192 && vec_ok(g, n) && vec_ok(x, ldx) && dw_floats >= static_cast<size_t>(2 * kCUs) * 64 * 64;
  }
};

// n == 1, the logit head: dx = g (x) w as a streaming store, dW / db as g-weighted column sums of x (fixed-order partials)
static int bwd_logit_head(const BwdCall& b) {
  const int k = b.k;
  if (b.dx != nullptr) {
    const bool vec = (k % 4 == 0) && (b.lddx % 4 == 0) &&
                     ((reinterpret_cast<uintptr_t>(b.dx) | reinterpret_cast<uintptr_t>(b.w)) & 15) == 0;
    const long long per_row = vec ? k / 4 : k;
    const unsigned blocks = outer_grid(static_cast<long long>(b.M) * per_row, per_row);
    if (vec) hipLaunchKernelGGL(outer_kernel<true>, dim3(blocks), dim3(256), 0, b.s, b.g, b.w, b.M, k, b.dx, b.lddx);
    else hipLaunchKernelGGL(outer_kernel<false>, dim3(blocks), dim3(256), 0, b.s, b.g, b.w, b.M, k, b.dx, b.lddx);
  }
  if (b.dw != nullptr || b.db != nullptr) {
    // row blocks: 1024 rows (the db partial area is sized for that), more when the dW partials would not fit
    const long long m = b.M;
    long long rpb = 1024;
    while (((m + rpb - 1) / rpb) * static_cast<long long>(k) > static_cast<long long>(b.dw_floats)) rpb *= 2;
    const int rb = static_cast<int>((m + rpb - 1) / rpb);
    hipLaunchKernelGGL(wcolsum_partial_kernel, dim3((k + 63) / 64, rb), dim3(256), 0, b.s, b.g, b.x, b.ldx, b.M, k,
                       static_cast<int>(rpb), b.ws, b.db_part());
    if (b.dw != nullptr)
      launch_splitk_reduce(b.s, static_cast<unsigned>((k + 63) / 64), b.ws, static_cast<long long>(k), rb, b.dw, b.db_part(), 1LL,
                           b.db);
    else if (b.db != nullptr)
      launch_splitk_reduce(b.s, 1u, b.db_part(), 1LL, rb, b.db);
  }
  return check_launch("logit head backward kernels");
}

// dW[64, 64] (+ db) of one 64-column half of g (ldg) in the slab form: partials per workgroup, then the fixed-order reduce
template <bool SCALED>
static void launch_tall_dw64(hipStream_t s, const float* g, long long ldg, const float* x, long long ldx, int M,
                             const float* row_scale, float* ws, float* db_part, float* dw, float* db) {
  const int n_wg = slab_grid(M);
  hipLaunchKernelGGL(tall_dw64_kernel<SCALED>, dim3(n_wg), dim3(64 * kSlabWaves), 0, s, g, ldg, x, ldx, M, ws, db_part, 0, row_scale);
  launch_splitk_reduce(s, 64u, ws, 64LL * 64, n_wg, dw, db_part, 64LL, db);
}

// The weight-gradient routes: each returns whether it took dW AND db, with the status in *rc.
// [m, 64]^T x [m, 64] over many rows: the slab kernel
static bool try_dw_slab64(const BwdCall& b, int* rc) {
  if (!(b.dw != nullptr && b.n == 64 && b.k == 64 && b.slab_ok())) return false;
  launch_tall_dw64<false>(b.s, b.g, b.n, b.x, b.ldx, b.M, nullptr, b.ws, b.db_part(), b.dw, b.db);
  *rc = check_launch("tall dW / db kernels (slab form)");
  return true;
}

// [m, 128]^T x [m, 64] (the fused K | V projection): the slab kernel once per 64-column half of g (x read twice: 840 MB
// of coalesced 1 KB requests against tall_dw_kernel<2>'s 630 MB of dword requests, 150 vs 199 us)
static bool try_dw_slab128x64(const BwdCall& b, int* rc) {
  if (!(b.dw != nullptr && b.n == 128 && b.k == 64 && b.slab_ok())) return false;
  for (int half = 0; half < 2; ++half)
    launch_tall_dw64<false>(b.s, b.g + 64 * half, b.n, b.x, b.ldx, b.M, nullptr, b.ws, b.db_part(),
                            b.dw + static_cast<long long>(half) * 64 * b.k, b.db != nullptr ? b.db + 64 * half : nullptr);
  *rc = check_launch("tall dW / db kernels (slab form, two halves)");
  return true;
}

// tall and narrow: one streaming pass over g and x leaves dW and db partials per workgroup (tall_dw_kernel)
static bool try_dw_tall(const BwdCall& b, int* rc) {
  if (!(b.dw != nullptr && b.n <= 256 && b.k <= 64 && b.M >= 8192)) return false;
  const int n = b.n, k = b.k;
  const long long m = b.M;
  long long n_wg = static_cast<long long>(b.dw_floats / (static_cast<size_t>(n) * k));
  if (n_wg > tall_wgs_max()) n_wg = tall_wgs_max();
  if (n_wg > (m + 63) / 64) n_wg = (m + 63) / 64;
  int rows_per_wg = static_cast<int>((m + n_wg - 1) / n_wg);
  rows_per_wg = (rows_per_wg + 15) / 16 * 16;
  n_wg = (m + rows_per_wg - 1) / rows_per_wg;
  float* dbp = b.db_part();
  const dim3 grid(static_cast<unsigned>(n_wg));
  const long long ldg = n;
  switch ((n + 63) / 64) {
    case 1: hipLaunchKernelGGL(tall_dw_kernel<1>, grid, dim3(256), 0, b.s, b.g, ldg, b.x, b.ldx, b.M, n, k, rows_per_wg, b.ws, dbp); break;
    case 2: hipLaunchKernelGGL(tall_dw_kernel<2>, grid, dim3(256), 0, b.s, b.g, ldg, b.x, b.ldx, b.M, n, k, rows_per_wg, b.ws, dbp); break;
    case 3: hipLaunchKernelGGL(tall_dw_kernel<3>, grid, dim3(256), 0, b.s, b.g, ldg, b.x, b.ldx, b.M, n, k, rows_per_wg, b.ws, dbp); break;
    default: hipLaunchKernelGGL(tall_dw_kernel<4>, grid, dim3(256), 0, b.s, b.g, ldg, b.x, b.ldx, b.M, n, k, rows_per_wg, b.ws, dbp); break;
  }
  const long long nk = static_cast<long long>(n) * k;
  launch_splitk_reduce(b.s, static_cast<unsigned>((nk + 63) / 64), b.ws, nk, static_cast<int>(n_wg), b.dw, dbp,
                       static_cast<long long>(n), b.db);       // dW and db in one launch
  *rc = check_launch("tall dW / db kernels");
  return true;
}

// everything else: dW through run_gemm (split K, or the split-operand kernel), db as column sums in 1024-row blocks
static int bwd_dw_db_generic(const BwdCall& b) {
  int rc = RBX_OK;
  if (b.dw != nullptr) {
    // dW[n,k] = g^T[n,m] * x[m,k]: A(i=n, kk=m) = g[m*n + n] (row contiguous), B(kk=m, col=k) = x[m*k + k]
    GemmCall c{b.g, b.n, b.x, b.ldx, b.dw, b.k, b.n, b.k, b.M, b.s};
    c.ws = b.ws;
    c.ws_floats = b.dw_floats;
    rc = run_gemm<false, false>(c);
    if (rc != RBX_OK) return rc;
  }
  if (b.db != nullptr) {
    const int rb = static_cast<int>((static_cast<long long>(b.M) + 1023) / 1024);
    hipLaunchKernelGGL(colsum_partial_kernel, dim3((b.n + 63) / 64, rb), dim3(256), 0, b.s, b.g, b.M, b.n, 1024, b.db_part());
    launch_splitk_reduce(b.s, static_cast<unsigned>((b.n + 63) / 64), b.db_part(), static_cast<long long>(b.n), rb, b.db);
    rc = check_launch("bias grad kernels");
  }
  return rc;
}

}  // namespace rbx

extern "C" int rbx_linear_fwd(const float* d_x, int64_t x_stride, const float* d_w, const float* d_bias, int64_t m,
                              int32_t n, int32_t k, int32_t act, float* d_y, void* stream) {
  if (m == 0) return RBX_OK;   // empty batch: nothing to do, pointers may be NULL
  using namespace rbx;
  if (d_x == nullptr || d_w == nullptr || d_y == nullptr) return fail(RBX_ERR_INVALID, "linear: NULL tensor");
  if (m < 0 || n <= 0 || k <= 0 || m > INT_MAX) return fail(RBX_ERR_INVALID, "linear: bad shape");
  if (x_stride < k) return fail(RBX_ERR_INVALID, "linear: x_stride %lld < k %d", static_cast<long long>(x_stride), k);
  if (act != 0 && act != 1) return fail(RBX_ERR_UNSUPPORTED, "linear: activation code %d", act);
  if (n == 1) {                                             // a logit head: one streaming pass, a wavefront per row
    long long blocks = (m + 3) / 4;
    if (blocks > kCUs * 16) blocks = kCUs * 16;
    const int vec = (x_stride % 4 == 0) && ((reinterpret_cast<uintptr_t>(d_x) | reinterpret_cast<uintptr_t>(d_w)) & 15) == 0;
    hipLaunchKernelGGL(gemv_fwd_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, as_stream(stream), d_x,
                       static_cast<long long>(x_stride), d_w, d_bias, static_cast<int>(m), k, act, vec, d_y);
    return check_launch("gemv_fwd_kernel");
  }
  return run_fwd_gemm(d_x, x_stride, d_w, d_bias, m, n, k, act, d_y, n, as_stream(stream), Epi{});
}

extern "C" int rbx_linear_fwd_fused(const float* d_x, int64_t x_stride, const float* d_w, const float* d_bias, int64_t m,
                                    int32_t n, int32_t k, int32_t act, const float* d_residual, int64_t residual_stride,
                                    const float* d_row_scale, float* d_y, int64_t y_stride, void* stream) {
  if (m == 0) return RBX_OK;
  using namespace rbx;
  if (d_x == nullptr || d_w == nullptr || d_y == nullptr) return fail(RBX_ERR_INVALID, "linear_fused: NULL tensor");
  if (m < 0 || n <= 1 || k <= 0 || m > INT_MAX) return fail(RBX_ERR_INVALID, "linear_fused: bad shape (n must be > 1)");
  if (x_stride < k || y_stride < n || (d_residual != nullptr && residual_stride < n))
    return fail(RBX_ERR_INVALID, "linear_fused: a row stride is shorter than its row");
  if (act != 0 && act != 1) return fail(RBX_ERR_UNSUPPORTED, "linear_fused: activation code %d", act);
  Epi epi{};
  epi.res = d_residual;
  epi.ldres = static_cast<long long>(residual_stride);
  epi.rowscale = d_row_scale;
  return run_fwd_gemm(d_x, x_stride, d_w, d_bias, m, n, k, act, d_y, y_stride, as_stream(stream), epi);
}

extern "C" int rbx_linear_dx_fused(const float* d_dy, int64_t dy_stride, const float* d_w, int64_t m, int32_t n, int32_t k,
                                   const float* d_mask, int64_t mask_stride, const float* d_residual,
                                   int64_t residual_stride, float* d_dx, int64_t dx_stride, void* stream) {
  if (m == 0) return RBX_OK;
  using namespace rbx;
  if (d_dy == nullptr || d_w == nullptr || d_dx == nullptr) return fail(RBX_ERR_INVALID, "linear_dx_fused: NULL tensor");
  if (m < 0 || n <= 0 || k <= 1 || m > INT_MAX) return fail(RBX_ERR_INVALID, "linear_dx_fused: bad shape (k must be > 1)");
  if (dy_stride < n || dx_stride < k || (d_mask != nullptr && mask_stride < k) ||
      (d_residual != nullptr && residual_stride < k))
    return fail(RBX_ERR_INVALID, "linear_dx_fused: a row stride is shorter than its row");
  Epi epi{};
  epi.res = d_residual;
  epi.ldres = static_cast<long long>(residual_stride);
  epi.mask = d_mask;
  epi.ldmask = static_cast<long long>(mask_stride);
  return run_dx_gemm(d_dy, dy_stride, d_w, m, n, k, d_dx, dx_stride, as_stream(stream), epi);
}

extern "C" int rbx_linear_dx_deepfm(const float* d_dy, int64_t dy_stride, const float* d_w, int64_t m, int32_t n, int32_t k,
                                    const float* d_x, int64_t x_stride, const float* d_fm_sum, int32_t fm_dim,
                                    int32_t fm_cols, const float* d_fm_g, const float* d_lr_g, const float* d_lr_w,
                                    float* d_dx, int64_t dx_stride, void* stream) {
  if (m == 0) return RBX_OK;
  using namespace rbx;
  if (!d_dy || !d_w || !d_dx || !d_x || !d_fm_sum || !d_fm_g) return fail(RBX_ERR_INVALID, "linear_dx_deepfm: NULL tensor");
  if ((d_lr_g == nullptr) != (d_lr_w == nullptr)) return fail(RBX_ERR_INVALID, "linear_dx_deepfm: lr_g and lr_w come together");
  if (m < 0 || n <= 0 || k <= 1 || m > INT_MAX || fm_dim <= 0 || fm_cols <= 0 || fm_cols > k || fm_cols % fm_dim != 0)
    return fail(RBX_ERR_INVALID, "linear_dx_deepfm: bad shape (fm_cols %d of k %d, fm_dim %d)", fm_cols, k, fm_dim);
  if (dy_stride < n || dx_stride < k || x_stride < fm_cols) return fail(RBX_ERR_INVALID, "linear_dx_deepfm: row stride too short");
  Epi epi{};
  epi.fm_x = d_x;
  epi.fm_ldx = static_cast<long long>(x_stride);
  epi.fm_s = d_fm_sum;
  epi.fm_g = d_fm_g;
  epi.lr_g = d_lr_g;
  epi.lr_w = d_lr_w;
  epi.fm_cols = fm_cols;
  epi.fm_dim = fm_dim;
  epi.fm_mask = (fm_dim & (fm_dim - 1)) == 0 ? fm_dim - 1 : -1;
  return run_dx_gemm(d_dy, dy_stride, d_w, m, n, k, d_dx, dx_stride, as_stream(stream), epi);
}

extern "C" size_t rbx_linear_bwd_workspace_size(int64_t m, int32_t n, int32_t k, int32_t act) {
  // relu-masked dy copy + split-K slices of dW (at most 2*CUs tiles worth) + bias partials
  const size_t masked = (act == 1) ? static_cast<size_t>(m) * n : 0;
  const size_t dw = rbx::dw_ws_floats(n, k);
  // bias partials: one row of n floats per 1024-row block -- or per workgroup of the tall-and-narrow kernel, whichever is more
  const size_t db_rows = static_cast<size_t>((m + 1023) / 1024) > static_cast<size_t>(rbx::tall_wgs_max())
                             ? static_cast<size_t>((m + 1023) / 1024) : static_cast<size_t>(rbx::tall_wgs_max());
  const size_t db = db_rows * n;
  return (masked + dw + db + 1024) * sizeof(float);
}

extern "C" int rbx_linear_bwd(const float* d_x, int64_t x_stride, const float* d_w, const float* d_y, const float* d_dy,
                              int64_t m, int32_t n, int32_t k, int32_t act, float* d_dx, int64_t dx_stride, float* d_dw,
                              float* d_db, void* d_workspace, size_t workspace_bytes, void* stream) {
  if (m == 0) return RBX_OK;   // empty batch: nothing to do, pointers may be NULL
  using namespace rbx;
  if (d_x == nullptr || d_w == nullptr || d_dy == nullptr) return fail(RBX_ERR_INVALID, "linear_bwd: NULL tensor");
  if (x_stride < k || (d_dx != nullptr && dx_stride < k)) return fail(RBX_ERR_INVALID, "linear_bwd: row stride < k");
  if (act == 1 && d_y == nullptr) return fail(RBX_ERR_INVALID, "linear_bwd: y is needed for the ReLU mask");
  if (m < 0 || m > INT_MAX) return fail(RBX_ERR_INVALID, "linear_bwd: bad m");
  const size_t need = rbx_linear_bwd_workspace_size(m, n, k, act);
  if (d_workspace == nullptr || workspace_bytes < need) return fail(RBX_ERR_WORKSPACE, "linear_bwd: workspace too small");
  hipStream_t s = as_stream(stream);
  float* ws = static_cast<float*>(d_workspace);
  const float* g = d_dy;
  if (act == 1) {
    const long long cnt = static_cast<long long>(m) * n;
    hipLaunchKernelGGL(relu_mask_kernel, dim3(capped_grid(cnt, 256)), dim3(256), 0, s, d_dy, d_y, cnt, ws);
    g = ws;
    ws += cnt;
  }
  const BwdCall b{g, d_x, x_stride, d_w, static_cast<int>(m), n, k, d_dx, dx_stride, d_dw, d_db, ws, dw_ws_floats(n, k), s};
  if (n == 1) return bwd_logit_head(b);
  int rc = RBX_OK;
  if (d_dx != nullptr) {
    rc = run_dx_gemm(g, n, d_w, m, n, k, d_dx, dx_stride, s, Epi{});
    if (rc != RBX_OK) return rc;
  }
  if (try_dw_slab64(b, &rc)) return rc;
  if (try_dw_slab128x64(b, &rc)) return rc;
  if (try_dw_tall(b, &rc)) return rc;
  return bwd_dw_db_generic(b);
}

// dW[64, 64] = (diag(row_scale) dy)^T x and db = its column sums in the slab kernel, the scaled gradient never written
// (the `seqs *= ~timeline_mask` of a SASRec block, sasrec.py:92, in the backward of the Linear in front of it)
extern "C" int rbx_linear_dwdb_scaled(const float* d_x, int64_t x_stride, const float* d_dy, int64_t dy_stride,
                                      const float* d_row_scale, int64_t m, int32_t n, int32_t k, float* d_dw, float* d_db,
                                      void* d_workspace, size_t workspace_bytes, void* stream) {
  if (m == 0) return RBX_OK;
  using namespace rbx;
  if (!d_x || !d_dy || !d_row_scale || !d_dw) return fail(RBX_ERR_INVALID, "linear_dwdb_scaled: NULL tensor");
  if (m < 0 || m > INT_MAX || x_stride < k || dy_stride < n) return fail(RBX_ERR_INVALID, "linear_dwdb_scaled: bad shape");
  const size_t need = rbx_linear_bwd_workspace_size(m, n, k, 0);
  if (d_workspace == nullptr || workspace_bytes < need) return fail(RBX_ERR_WORKSPACE, "linear_dwdb_scaled: workspace too small");
  const size_t dw_floats = dw_ws_floats(n, k);
  if (!(n == 64 && k == 64 && m >= 8192 && vec_ok(d_dy, dy_stride) && vec_ok(d_x, x_stride) &&
        dw_floats >= static_cast<size_t>(2 * kCUs) * 64 * 64))
    return fail(RBX_ERR_UNSUPPORTED, "linear_dwdb_scaled: only [m >= 8192, 64]^T x [m, 64] with 16-byte aligned rows");
  float* ws = static_cast<float*>(d_workspace);
  launch_tall_dw64<true>(as_stream(stream), d_dy, dy_stride, d_x, x_stride, static_cast<int>(m), d_row_scale, ws,
                         d_db != nullptr ? ws + dw_floats : nullptr, d_dw, d_db);
  return check_launch("tall dW / db kernels (slab form, scaled rows)");
}

extern "C" int rbx_linear_dx_scaled(const float* d_dy, int64_t dy_stride, const float* d_w, int64_t m, int32_t n, int32_t k,
                                    const float* d_mask, int64_t mask_stride, const float* d_residual,
                                    int64_t residual_stride, const float* d_row_scale, float* d_dx, int64_t dx_stride,
                                    void* stream) {
  if (m == 0) return RBX_OK;
  using namespace rbx;
  if (d_dy == nullptr || d_w == nullptr || d_dx == nullptr || d_row_scale == nullptr)
    return fail(RBX_ERR_INVALID, "linear_dx_scaled: NULL tensor");
  if (m < 0 || n <= 0 || k <= 1 || m > INT_MAX) return fail(RBX_ERR_INVALID, "linear_dx_scaled: bad shape (k must be > 1)");
  if (dy_stride < n || dx_stride < k || (d_mask != nullptr && mask_stride < k) ||
      (d_residual != nullptr && residual_stride < k))
    return fail(RBX_ERR_INVALID, "linear_dx_scaled: a row stride is shorter than its row");
  Epi epi{};
  epi.res = d_residual;
  epi.ldres = static_cast<long long>(residual_stride);
  epi.mask = d_mask;
  epi.ldmask = static_cast<long long>(mask_stride);
  epi.rowscale = d_row_scale;
  return run_dx_gemm(d_dy, dy_stride, d_w, m, n, k, d_dx, dx_stride, as_stream(stream), epi);
}

// ---- bf16 planes of a weight matrix for the split-operand GEMM (see gemm_bx6_kernel) -------------------------------------
extern "C" size_t rbx_split_bf16_size(int32_t rows, int32_t cols, int32_t transpose) {
  if (rows <= 0 || cols <= 0) return 0;
  const long long orows = transpose ? cols : rows, ocols = transpose ? rows : cols;
  const long long cp = (ocols + rbx::SBK - 1) / rbx::SBK * rbx::SBK;
  return static_cast<size_t>(3 * orows * cp * 2);
}

extern "C" int rbx_split_bf16(const float* d_src, int64_t ld, int32_t rows, int32_t cols, int32_t transpose, void* d_out,
                              void* stream) {
  using namespace rbx;
  if (rows <= 0 || cols <= 0) return RBX_OK;
  if (d_src == nullptr || d_out == nullptr || ld < cols) return fail(RBX_ERR_INVALID, "split_bf16: bad arguments");
  if ((reinterpret_cast<uintptr_t>(d_out) & 15) != 0) return fail(RBX_ERR_INVALID, "split_bf16: output must be 16-byte aligned");
  const long long pairs = static_cast<long long>(rbx_split_bf16_size(rows, cols, transpose) / 12);
  hipLaunchKernelGGL(split_bf16_kernel, dim3(capped_grid(pairs, 256)), dim3(256), 0, as_stream(stream), d_src,
                     static_cast<long long>(ld), rows, cols, transpose, static_cast<unsigned short*>(d_out));
  return check_launch("split_bf16_kernel");
}

extern "C" int rbx_split_register(const float* d_w, const void* d_planes, int32_t rows, int32_t cols, int32_t transposed) {
  using namespace rbx;
  if (d_w == nullptr || d_planes == nullptr || rows <= 0 || cols <= 0) return fail(RBX_ERR_INVALID, "split_register: bad arguments");
  std::lock_guard<std::mutex> lock(g_split_mu);
  int slot = -1;
  for (int i = 0; i < kSplitSlots; ++i)
    if (g_split[i].w == d_w && g_split[i].transposed == (transposed ? 1 : 0)) slot = i;
  for (int i = 0; i < kSplitSlots && slot < 0; ++i)
    if (g_split[i].planes == nullptr) slot = i;
  if (slot < 0) return fail(RBX_ERR_UNSUPPORTED, "split_register: all %d slots are taken", kSplitSlots);
  g_split[slot] = SplitEntry{d_w, static_cast<const unsigned short*>(d_planes), rows, cols, transposed ? 1 : 0};
  return RBX_OK;
}

extern "C" uint64_t rbx_gemm_bx6_count(void) { return rbx::g_bx6_launches.load(std::memory_order_relaxed); }

extern "C" int rbx_split_unregister(const float* d_w) {
  using namespace rbx;
  std::lock_guard<std::mutex> lock(g_split_mu);
  for (int i = 0; i < kSplitSlots; ++i)
    if (g_split[i].w == d_w) g_split[i] = SplitEntry{nullptr, nullptr, 0, 0, 0};
  return RBX_OK;
}
