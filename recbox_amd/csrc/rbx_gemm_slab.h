// rbx_gemm_slab.h -- the kernels of rbx_dense.hip that are no 128 x 128 tile: the fixed-order reduce of split-K partials, the
// ReLU mask and column sums of the backward, the logit heads (n = 1), the tall-and-narrow weight gradients and the slab
// kernels that stream [M, 64 / 128] activations past weights held in registers or LDS.  Included by rbx_dense.hip.
#pragma once
#include <type_traits>
#include "rbx_internal.h"
#include "rbx_gemm_tile.h"

namespace rbx {

// C[i] = sum_z part[z][i] in a fixed order.  A workgroup owns 64 outputs; its 4 wavefronts take every 4th slice
// (4 independent partial sums each, so the loads overlap) and meet in LDS.  The earlier one-thread-per-output
// loop ran 148 us for 512 slices of a [64, 64] weight gradient: 16 workgroups of dependent loads.
constexpr int kRedZ = 16;                  // slices summed side by side per output (wavefronts of the reduce workgroup)
__global__ __launch_bounds__(64 * kRedZ) void splitk_reduce_kernel(const float* __restrict__ part, const long long n,
                                                                    const int splits, float* __restrict__ out,
                                                                    const float* __restrict__ part2, const long long n2,
                                                                    float* __restrict__ out2, const int blocks1) {
  // (part2, n2, out2): a second, smaller reduction over the same number of slices rides in the same launch -- the bias
  // partials beside the weight partials -- in the workgroups from blocks1 on
  __shared__ float red[kRedZ][64];
  const int col = threadIdx.x & 63, zl = threadIdx.x >> 6;
  const bool second = static_cast<int>(blockIdx.x) >= blocks1;
  const float* src = second ? part2 : part;
  float* dst = second ? out2 : out;
  const long long nn = second ? n2 : n;
  const long long b0 = second ? blockIdx.x - blocks1 : blockIdx.x;
  const long long nb = second ? gridDim.x - blocks1 : blocks1;
  for (long long i0 = b0 * 64; i0 < nn; i0 += nb * 64) {
    const long long i = i0 + col;
    float t0 = 0.f, t1 = 0.f, t2 = 0.f, t3 = 0.f;
    if (i < nn) {
      int z = zl;
      for (; z + 3 * kRedZ < splits; z += 4 * kRedZ) {
        t0 += src[static_cast<long long>(z) * nn + i];
        t1 += src[static_cast<long long>(z + kRedZ) * nn + i];
        t2 += src[static_cast<long long>(z + 2 * kRedZ) * nn + i];
        t3 += src[static_cast<long long>(z + 3 * kRedZ) * nn + i];
      }
      for (; z < splits; z += kRedZ) t0 += src[static_cast<long long>(z) * nn + i];
    }
    red[zl][col] = (t0 + t1) + (t2 + t3);
    __syncthreads();
    if (zl == 0 && i < nn) {
      float t = 0.f;
#pragma unroll
      for (int w = 0; w < kRedZ; ++w) t += red[w][col];
      dst[i] = t;
    }
    __syncthreads();
  }
}

// dy' = dy * (y > 0)   (ReLU backward, in a scratch buffer so dy stays intact)
__global__ __launch_bounds__(256) void relu_mask_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                                        const long long n, float* __restrict__ out) {
  const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
  for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride)
    out[i] = y[i] > 0.f ? dy[i] : 0.f;
}

// column sums of dy[M,N]: grid (ceil(N/64), row_blocks); partial[rb][n]
__global__ __launch_bounds__(256) void colsum_partial_kernel(const float* __restrict__ dy, const int M, const int N,
                                                             const int rows_per_block, float* __restrict__ partial) {
  __shared__ float red[4][64];
  const int n = blockIdx.x * 64 + (threadIdx.x & 63);
  const int r0 = blockIdx.y * rows_per_block;
  const int r1 = (r0 + rows_per_block < M) ? r0 + rows_per_block : M;
  float t = 0.f;
  if (n < N) {
    int r = r0 + (threadIdx.x >> 6);
    for (; r + 28 < r1; r += 32) {                           // 8 rows in flight, added in the same (ascending) order
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = dy[static_cast<long long>(r + 4 * u) * N + n];
#pragma unroll
      for (int u = 0; u < 8; ++u) t += v[u];
    }
    for (; r < r1; r += 4) t += dy[static_cast<long long>(r) * N + n];
  }
  red[threadIdx.x >> 6][threadIdx.x & 63] = t;
  __syncthreads();
  if (threadIdx.x < 64 && n < N)
    partial[static_cast<long long>(blockIdx.y) * N + n] = (red[0][threadIdx.x] + red[1][threadIdx.x]) +
                                                          (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// ---- n == 1: the logit heads (Linear(400, 1) of every tower, rechub LR's Linear(F*D, 1)) -----------------------------
// A [M, K] x [K] product is a streaming read of x; on the 128 x 32 narrow GEMM tile it ran at 2.6 TB/s ([65 536, 1664]:
// 168 us forward, 480 us backward).  Here: a wavefront per row with a fixed xor butterfly (forward), an outer product
// whose lanes keep their columns of w in registers (dx), and g-weighted column sums with fixed-order partials (dW, db).
__global__ __launch_bounds__(256) void gemv_fwd_kernel(const float* __restrict__ x, const long long ldx,
                                                       const float* __restrict__ w, const float* __restrict__ bias,
                                                       const int M, const int K, const int act, const int vec,
                                                       float* __restrict__ y) {
  const int lane = threadIdx.x & 63;
  const int nwaves = gridDim.x * 4;
  const int k4 = vec ? (K & ~3) : 0;
  for (int r = blockIdx.x * 4 + (threadIdx.x >> 6); r < M; r += nwaves) {
    const float* __restrict__ xr = x + static_cast<long long>(r) * ldx;
    float acc = 0.f;
#pragma unroll 4
    for (int c = lane * 4; c < k4; c += 256) {
      const float4 a = *reinterpret_cast<const float4*>(xr + c);
      const float4 b = *reinterpret_cast<const float4*>(w + c);
      acc += (a.x * b.x + a.y * b.y) + (a.z * b.z + a.w * b.w);
    }
#pragma unroll 4
    for (int c = k4 + lane; c < K; c += 64) acc += xr[c] * w[c];
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) {
      float v = acc + (bias != nullptr ? bias[0] : 0.f);
      if (act == 1 && v < 0.f) v = 0.f;
      y[r] = v;
    }
  }
}

// dx[r, c] = g[r] * w[c].  VEC: K % 4 == 0, 16-byte aligned rows.  When the grid stride is a multiple of the row length
// (outer_grid) a lane keeps its columns; otherwise it recomputes (row, column) per element.
template <bool VEC>
__global__ __launch_bounds__(256) void outer_kernel(const float* __restrict__ g, const float* __restrict__ w, const int M,
                                                    const int K, float* __restrict__ dx, const long long lddx) {
  constexpr int W = VEC ? 4 : 1;
  const unsigned per_row = static_cast<unsigned>(K / W);
  const long long total = static_cast<long long>(M) * per_row;
  const long long step = static_cast<long long>(gridDim.x) * blockDim.x;
  long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= total) return;
  if (step % per_row == 0) {
    long long r = i / per_row;
    const int c = static_cast<int>(i - r * per_row) * W;
    const long long dr = step / per_row;
    float wv[W];
#pragma unroll
    for (int q = 0; q < W; ++q) wv[q] = w[c + q];
#pragma unroll 4
    for (; r < M; r += dr) {
      const float gr = g[r];
      float* dst = dx + r * lddx + c;
      if constexpr (VEC) *reinterpret_cast<float4*>(dst) = make_float4(gr * wv[0], gr * wv[1], gr * wv[2], gr * wv[3]);
      else dst[0] = gr * wv[0];
    }
    return;
  }
  for (; i < total; i += step) {
    const long long r = i / per_row;
    const int c = static_cast<int>(i - r * per_row) * W;
    const float gr = g[r];
    float* dst = dx + r * lddx + c;
    if constexpr (VEC) *reinterpret_cast<float4*>(dst) = make_float4(gr * w[c], gr * w[c + 1], gr * w[c + 2], gr * w[c + 3]);
    else dst[0] = gr * w[c];
  }
}

// dw_part[rb][k] = sum over the row block of g[r] * x[r, k]; db_part[rb] = sum of g[r]: grid (ceil(K/64), row_blocks)
__global__ __launch_bounds__(256) void wcolsum_partial_kernel(const float* __restrict__ g, const float* __restrict__ x,
                                                              const long long ldx, const int M, const int K,
                                                              const int rows_per_block, float* __restrict__ dw_part,
                                                              float* __restrict__ db_part) {
  __shared__ float red[4][64];
  __shared__ float redg[4];
  const int n = blockIdx.x * 64 + (threadIdx.x & 63);
  const int r0 = blockIdx.y * rows_per_block;
  const int r1 = (r0 + rows_per_block < M) ? r0 + rows_per_block : M;
  const bool ok = n < K;
  float t = 0.f, gs = 0.f;
  int r = r0 + (threadIdx.x >> 6);
  for (; r + 28 < r1; r += 32) {                             // 8 rows in flight, added in ascending order
    float v[8], gg[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      gg[u] = g[r + 4 * u];
      v[u] = ok ? x[static_cast<long long>(r + 4 * u) * ldx + n] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      t += gg[u] * v[u];
      gs += gg[u];
    }
  }
  for (; r < r1; r += 4) {
    const float gr = g[r];
    t += gr * (ok ? x[static_cast<long long>(r) * ldx + n] : 0.f);
    gs += gr;
  }
  red[threadIdx.x >> 6][threadIdx.x & 63] = t;
  if ((threadIdx.x & 63) == 0) redg[threadIdx.x >> 6] = gs;
  __syncthreads();
  if (threadIdx.x < 64 && ok)
    dw_part[static_cast<long long>(blockIdx.y) * K + n] = (red[0][threadIdx.x] + red[1][threadIdx.x]) +
                                                          (red[2][threadIdx.x] + red[3][threadIdx.x]);
  if (threadIdx.x == 0 && blockIdx.x == 0 && db_part != nullptr)
    db_part[blockIdx.y] = (redg[0] + redg[1]) + (redg[2] + redg[3]);
}

// dW[n,k] = g^T x (and db = column sums of g) for a TALL, NARROW layer -- n <= 256, k <= 64 with hundreds of thousands of rows
// (SASRec's [B*L, 64] x [64, 64] and fused [64 -> 192] projections): a streaming reduction over the rows, bound by reading g and x once.
// The four wavefronts of a workgroup own the four 32 x 32 quadrants of dW; a lane feeds v_mfma_f32_32x32x2_f32 straight
// from global memory -- A[i][kk] = g[r + kk][c0 + i], B[kk][j] = x[r + kk][d0 + j]: lanes 0..31 read 128 contiguous bytes
// of row r, lanes 32..63 of row r + 1 -- with 8 row pairs in flight, no LDS staging.  Every workgroup leaves a partial
// [n, k] (and [n]) that splitk_reduce_kernel sums in a fixed order.  (The general split-K tile kernel spent 285 us on
// [819200, 64]^T x [819200, 64]: a quarter-filled 128 x 128 tile per workgroup; its column-sum companion 107 us.)
template <int NQ>
__global__ __launch_bounds__(256) void tall_dw_kernel(const float* __restrict__ g, const long long ldg,
                                                      const float* __restrict__ x, const long long ldx, const int M,
                                                      const int n, const int k, const int rows_per_wg,
                                                      float* __restrict__ dw_part, float* __restrict__ db_part) {
  // wavefront w: x columns d0 = (w & 1) * 32 .. + 32 against the g column blocks (w >> 1) + 2 q, q < NQ (n <= 64 NQ)
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int li = lane & 31, lk = lane >> 5;
  const int d0 = (wid & 1) * 32;
  const bool d_ok = d0 + li < k;
  const int r_beg = blockIdx.x * rows_per_wg;
  const int r_end = (r_beg + rows_per_wg < M) ? r_beg + rows_per_wg : M;
  f32x16 acc[NQ];
  float colsum[NQ];
  bool c_ok[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;
    colsum[q] = 0.f;
    c_ok[q] = ((wid >> 1) + 2 * q) * 32 + li < n;
  }
  constexpr int U = (NQ == 1) ? 8 : 4;     // row pairs in flight (a wavefront feeding both x halves from one g load was slower)
  const float* gp = g + (wid >> 1) * 32 + li;
  const float* xp = x + d0 + li;
  for (int r0 = r_beg; r0 < r_end; r0 += 2 * U) {
    float a[NQ][U], b[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int r = r0 + 2 * u + lk;
      const bool in = r < r_end;
      b[u] = (in && d_ok) ? xp[static_cast<long long>(r) * ldx] : 0.f;
#pragma unroll
      for (int q = 0; q < NQ; ++q) a[q][u] = (in && c_ok[q]) ? gp[static_cast<long long>(r) * ldg + q * 64] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q][u], b[u], acc[q], 0, 0, 0);
        colsum[q] += a[q][u];
      }
    }
  }
  // C/D layout of the 32x32 MFMA: col = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
  float* out = dw_part + static_cast<long long>(blockIdx.x) * n * k;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int c0 = ((wid >> 1) + 2 * q) * 32;
    if (d_ok) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = c0 + (r & 3) + 8 * (r >> 2) + 4 * lk;
        if (row < n) out[row * k + d0 + li] = acc[q][r];
      }
    }
    if (db_part != nullptr && (wid & 1) == 0) {            // the wavefronts of x-quadrant 0 also own the column sums
      const float t = colsum[q] + __shfl_xor(colsum[q], 32, 64);
      if (lk == 0 && c_ok[q]) db_part[static_cast<long long>(blockIdx.x) * n + c0 + li] = t;
    }
  }
}

// ---- K = 64, N = 64 over hundreds of thousands of rows: the weights live in REGISTERS ------------------------------------
// SASRec's projections and FFN convolutions (sasrec.py:81-94,110-124) are [B*L, 64] x [64, 64]: 6.7 GFLOP against 420 MB of
// activations, a streaming pass.  On the staged tile kernel above they ran at 3.3-3.6 TB/s (four k tiles of 16, a barrier
// each, W re-staged per 128 rows).  Here a wavefront owns 32-row slabs and never meets the others.  The k index a lane
// feeds to v_mfma_f32_32x32x2_f32 may be ANY pairing the two operands agree on: lane (m, h) = (lane % 32, lane / 32) holds
// floats [32 h, 32 h + 32) of row m and MFMA step j takes k = 32 h + j against W(k, n), which sits in 2 x 32 registers per
// lane for the whole kernel.  A slab is fetched as eight fully coalesced 1 KB requests (four rows each; per-lane 128-byte
// reads of 64 different lines thrashed the L1: 8x the L2 traffic, slower than the tile kernel), turned into that layout
// through a wavefront-private 8 KB of LDS (no barrier), and the next slab's requests are in flight under the current
// slab's 64 MFMAs.  MFMA-bound rate: 64 x 64 cycles per slab and SIMD = 9.6 TB/s of traffic, above what HBM delivers.
// The residual / mask operands are read with `nt` loads, the outputs go out as plain stores: measured on SASRec
// (profiles/r03), plain stores 10.27 ms against streamed stores 10.33, `nt` operands 10.27 against 10.35.
constexpr int kSlabWaves = 4;              // wavefronts per workgroup (independent of each other)
constexpr int kSlabLd = 64 + 4;            // LDS row pitch of a slab (floats): b128 reads of 32 rows spread over the banks
// A slab = 32 rows of 64 floats, fetched as eight 1 KB requests: request p covers rows 4 p .. 4 p + 3, lane l takes floats
// [4 (l % 16), + 4) of row 4 p + l / 16.  The per-lane byte offsets below are the same for every full slab (computed once);
// the slab's first row comes in as a wave-uniform base (SGPR pair), so a request costs no vector arithmetic at all -- the
// first version spent ~600 integer instructions per slab on 64-bit row addresses and per-row bounds tests, as long as
// the 64 MFMAs themselves (profiles/r03: 70 % of the wavefront cycles were issue stalls, the MFMA pipes 0.43 busy).
__device__ __forceinline__ void slab_offsets(long long ld, int rows_left, int lane, unsigned (&off)[8]) {
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    int row = 4 * p + (lane >> 4);
    row = row < rows_left ? row : rows_left - 1;         // (the last, partial slab re-reads its last row)
    off[p] = static_cast<unsigned>((static_cast<long long>(row) * ld + 4 * (lane & 15)) * 4);
  }
}
__device__ __forceinline__ void slab_issue(const float* base, const unsigned (&off)[8], f32x4 (&v)[8]) {
#pragma unroll
  for (int p = 0; p < 8; ++p) asm volatile("global_load_dwordx4 %0, %1, %2 nt" : "=v"(v[p]) : "v"(off[p]), "s"(base));
}
__device__ __forceinline__ void slab_arrived(f32x4 (&v)[8]) {
  asm volatile("s_waitcnt vmcnt(0)"
               : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]), "+v"(v[7])
               :
               : "memory");
}
// registers of slab_issue -> the lane's half row, through the wavefront's LDS slab
__device__ __forceinline__ void slab_turn(float* __restrict__ lds, int lane, const f32x4 (&v)[8], float (&a)[32]) {
  float* dst = lds + (lane >> 4) * kSlabLd + 4 * (lane & 15);
#pragma unroll
  for (int p = 0; p < 8; ++p) *reinterpret_cast<f32x4*>(dst + 4 * p * kSlabLd) = v[p];
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const float* src = lds + (lane & 31) * kSlabLd + 32 * (lane >> 5);
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const f32x4 u = *reinterpret_cast<const f32x4*>(src + 4 * q);
    a[4 * q] = u[0]; a[4 * q + 1] = u[1]; a[4 * q + 2] = u[2]; a[4 * q + 3] = u[3];
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();         // (the next slab_turn overwrites what these reads fetch)
}
// element (i, t) of a wavefront's two 32 x 32 output tiles sits in row (i & 3) + 8 (i >> 2) + 4 h, column 32 t + m
__device__ __forceinline__ constexpr int slab_row(int i) { return (i & 3) + 8 * (i >> 2); }

// EPI: 1 residual, 2 mask, 4 row scale, 8 ReLU -- compile-time, so that a launch carries only its own epilogue
template <bool B_KCONTIG, int EPI>
__global__ __launch_bounds__(64 * kSlabWaves, 2) void gemm_f32_k64n64_kernel(
    const float* __restrict__ A, const long long lda, const float* __restrict__ B, const long long ldb, float* __restrict__ C,
    const long long ldc, const int M, const float* __restrict__ bias, const Epi epi) {
  __shared__ float slab[kSlabWaves][32 * kSlabLd];
  const int lane = threadIdx.x & 63, m = lane & 31, h = lane >> 5;
  const int wid = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));      // wave-uniform, and known to be
  const int nw = static_cast<int>(gridDim.x) * kSlabWaves;
  const int slabs = (M + 31) >> 5;
  int s = static_cast<int>(blockIdx.x) * kSlabWaves + wid;
  if (s >= slabs) return;
  float* lds = slab[wid];
  unsigned off_full[8], off[8];
  slab_offsets(lda, 32, lane, off_full);
  f32x4 nx[8];
  {
    const int left = M - s * 32;
#pragma unroll
    for (int p = 0; p < 8; ++p) off[p] = off_full[p];
    if (left < 32) slab_offsets(lda, left, lane, off);
    slab_issue(A + static_cast<long long>(s) * 32 * lda, off, nx);
  }
  // W(k = 32 h + j, n = 32 t + m), t = 0, 1
  float w0[32], w1[32];
  if constexpr (B_KCONTIG) {               // B(k, n) = B[n * ldb + k]: 32 consecutive floats of rows m and 32 + m
    const float4* p0 = reinterpret_cast<const float4*>(B + static_cast<long long>(m) * ldb + 32 * h);
    const float4* p1 = reinterpret_cast<const float4*>(B + static_cast<long long>(32 + m) * ldb + 32 * h);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const float4 u = p0[q], v = p1[q];
      w0[4 * q] = u.x; w0[4 * q + 1] = u.y; w0[4 * q + 2] = u.z; w0[4 * q + 3] = u.w;
      w1[4 * q] = v.x; w1[4 * q + 1] = v.y; w1[4 * q + 2] = v.z; w1[4 * q + 3] = v.w;
    }
  } else {                                 // B(k, n) = B[k * ldb + n]
#pragma unroll
    for (int j = 0; j < 32; ++j) {
      const float* r = B + static_cast<long long>(32 * h + j) * ldb + m;
      w0[j] = r[0];
      w1[j] = r[32];
    }
  }
  const float b0 = bias != nullptr ? bias[m] : 0.f, b1 = bias != nullptr ? bias[32 + m] : 0.f;
  constexpr bool has_res = (EPI & 1) != 0, has_mask = (EPI & 2) != 0, has_rs = (EPI & 4) != 0, relu = (EPI & 8) != 0;
  // per-lane parts of the epilogue's addresses (bytes): row 4 h of the slab, column m
  const long long c_lane = (4LL * h * ldc + m) * 4;
  const long long res_lane = has_res ? (4LL * h * epi.ldres + m) * 4 : 0;
  const long long msk_lane = has_mask ? (4LL * h * epi.ldmask + m) * 4 : 0;
  float a[32];
  slab_arrived(nx);
  slab_turn(lds, lane, nx, a);
  for (;;) {
    const int r0 = s * 32;
    int sn = s + nw;
    const bool more = sn < slabs;
    sn = more ? sn : s;                    // (the last round re-requests its own slab: no branch around the asm)
    {
      const int left = M - sn * 32;
#pragma unroll
      for (int p = 0; p < 8; ++p) off[p] = off_full[p];
      if (left < 32) slab_offsets(lda, left, lane, off);
      slab_issue(A + static_cast<long long>(sn) * 32 * lda, off, nx);
    }
    const int left = M - r0;               // rows of this slab that exist (wave-uniform)
    const bool full = left >= 32;
    // the epilogue's operands are fetched now, under the MFMAs
    f32x16 res0, res1, msk0, msk1;
    float rs[16];
    if constexpr (has_res) {
      const char* base = reinterpret_cast<const char*>(epi.res + static_cast<long long>(r0) * epi.ldres) + res_lane;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int k = (full || slab_row(i) + 4 * h < left) ? slab_row(i) : 0;
        const float* q = reinterpret_cast<const float*>(base + static_cast<long long>(k) * epi.ldres * 4);
        res0[i] = __builtin_nontemporal_load(q);
        res1[i] = __builtin_nontemporal_load(q + 32);
      }
    }
    if constexpr (has_mask) {
      const char* base = reinterpret_cast<const char*>(epi.mask + static_cast<long long>(r0) * epi.ldmask) + msk_lane;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int k = (full || slab_row(i) + 4 * h < left) ? slab_row(i) : 0;
        const float* q = reinterpret_cast<const float*>(base + static_cast<long long>(k) * epi.ldmask * 4);
        msk0[i] = __builtin_nontemporal_load(q);
        msk1[i] = __builtin_nontemporal_load(q + 32);
      }
    }
    if constexpr (has_rs) {
      // the slab's 32 row scales as ONE request (lane l: row l), dealt to the rows a lane finishes through the LDS crossbar:
      // sixteen loads of two distinct words each per slab made the kernel 40 us slower (147 vs 107 us at 819 200 rows) --
      // these kernels are bound by the number of memory requests, not by bytes
      const int rr = r0 + (lane & 31);
      const float mine = epi.rowscale[rr < M ? rr : M - 1];
#pragma unroll
      for (int i = 0; i < 16; ++i) rs[i] = __shfl(mine, slab_row(i) + 4 * h, 64);
    }
    f32x16 acc0, acc1;
#pragma unroll
    for (int i = 0; i < 16; ++i) { acc0[i] = 0.f; acc1[i] = 0.f; }
#pragma unroll
    for (int j = 0; j < 32; ++j) {
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], w0[j], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], w1[j], acc1, 0, 0, 0);
    }
    char* cbase = reinterpret_cast<char*>(C + static_cast<long long>(r0) * ldc) + c_lane;
    auto finish = [&](auto guarded) {        // two copies of the epilogue: full slabs store without a test per row
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        float v0 = acc0[i] + b0, v1 = acc1[i] + b1;
        if constexpr (relu) { v0 = v0 > 0.f ? v0 : 0.f; v1 = v1 > 0.f ? v1 : 0.f; }
        if constexpr (has_mask) { v0 = msk0[i] > 0.f ? v0 : 0.f; v1 = msk1[i] > 0.f ? v1 : 0.f; }
        if constexpr (has_res) { v0 += res0[i]; v1 += res1[i]; }
        if constexpr (has_rs) { v0 *= rs[i]; v1 *= rs[i]; }
        if (!decltype(guarded)::value || slab_row(i) + 4 * h < left) {
          float* q = reinterpret_cast<float*>(cbase + static_cast<long long>(slab_row(i)) * ldc * 4);
          q[0] = v0;
          q[32] = v1;
        }
      }
    };
    if (full) finish(std::false_type{});
    else finish(std::true_type{});
    slab_arrived(nx);
    if (!more) break;
    slab_turn(lds, lane, nx, a);
    s = sn;
  }
}

// The same slab form for [M, 64] x [64 -> 128] (NT = 4: SASRec's fused K | V projection, sasrec.py:81-87 via
// nn.MultiheadAttention's in_proj) and [M, 128] x [128 -> 64] (KH = 2: its dx): W no longer fits the registers beside the
// slab, so it sits in LDS once per workgroup ([k][n], 33-35 KB) and an MFMA step reads its B operand from there (one b32
// per lane: 32 consecutive floats per half-wave, conflict-free).  A 128-wide row is fetched as two 64-wide halves (each
// request still covers whole 256-byte runs) and turned one after the other through the same 8.5 KB of LDS, their products
// landing in the same accumulators.  Epilogue: bias, ReLU, residual.
template <int KH, int NT, bool B_KCONTIG, bool HAS_RES>
__global__ __launch_bounds__(64 * kSlabWaves, 2) void gemm_f32_slabw_kernel(
    const float* __restrict__ A, const long long lda, const float* __restrict__ B, const long long ldb, float* __restrict__ C,
    const long long ldc, const int M, const float* __restrict__ bias, const int act, const Epi epi) {
  constexpr int K = 64 * KH, N = 32 * NT, WLD = N + 4;
  __shared__ float slab[kSlabWaves][32 * kSlabLd];
  __shared__ float wl[K * WLD];
  for (int e = threadIdx.x; e < K * N; e += 64 * kSlabWaves) {
    int k, n;
    if constexpr (B_KCONTIG) { n = e / K; k = e % K; }       // B(k, n) = B[n * ldb + k]
    else { k = e / N; n = e % N; }                           // B(k, n) = B[k * ldb + n]
    wl[k * WLD + n] = B_KCONTIG ? B[static_cast<long long>(n) * ldb + k] : B[static_cast<long long>(k) * ldb + n];
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, m = lane & 31, h = lane >> 5;
  const int wid = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  const int nw = static_cast<int>(gridDim.x) * kSlabWaves;
  const int slabs = (M + 31) >> 5;
  int s = static_cast<int>(blockIdx.x) * kSlabWaves + wid;
  if (s >= slabs) return;
  float* lds = slab[wid];
  unsigned off_full[8], off[8];
  slab_offsets(lda, 32, lane, off_full);
  f32x4 nx[KH][8];
  auto issue = [&](int sl) {
    const int left = M - sl * 32;
#pragma unroll
    for (int p = 0; p < 8; ++p) off[p] = off_full[p];
    if (left < 32) slab_offsets(lda, left, lane, off);
#pragma unroll
    for (int hf = 0; hf < KH; ++hf) slab_issue(A + static_cast<long long>(sl) * 32 * lda + 64 * hf, off, nx[hf]);
  };
  auto arrived = [&]() {
#pragma unroll
    for (int hf = 0; hf < KH; ++hf) slab_arrived(nx[hf]);
  };
  issue(s);
  float bv[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) bv[t] = bias != nullptr ? bias[32 * t + m] : 0.f;
  const long long c_lane = (4LL * h * ldc + m) * 4;
  const long long res_lane = HAS_RES ? (4LL * h * epi.ldres + m) * 4 : 0;
  const float* wp = wl + 32 * h * WLD + m;
  float a[KH][32];
  arrived();
#pragma unroll
  for (int hf = 0; hf < KH; ++hf) slab_turn(lds, lane, nx[hf], a[hf]);
  for (;;) {
    const int r0 = s * 32;
    int sn = s + nw;
    const bool more = sn < slabs;
    sn = more ? sn : s;
    issue(sn);
    const int left = M - r0;
    const bool full = left >= 32;
    f32x16 res[NT];
    if constexpr (HAS_RES) {
      const char* base = reinterpret_cast<const char*>(epi.res + static_cast<long long>(r0) * epi.ldres) + res_lane;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int k = (full || slab_row(i) + 4 * h < left) ? slab_row(i) : 0;
        const float* q = reinterpret_cast<const float*>(base + static_cast<long long>(k) * epi.ldres * 4);
#pragma unroll
        for (int t = 0; t < NT; ++t) res[t][i] = __builtin_nontemporal_load(q + 32 * t);
      }
    }
    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
#pragma unroll
    for (int hf = 0; hf < KH; ++hf)
#pragma unroll
      for (int j = 0; j < 32; ++j)
#pragma unroll
        for (int t = 0; t < NT; ++t)
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[hf][j], wp[(64 * hf + j) * WLD + 32 * t], acc[t], 0, 0, 0);
    char* cbase = reinterpret_cast<char*>(C + static_cast<long long>(r0) * ldc) + c_lane;
    auto finish = [&](auto guarded) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        if (!decltype(guarded)::value || slab_row(i) + 4 * h < left) {
          float* q = reinterpret_cast<float*>(cbase + static_cast<long long>(slab_row(i)) * ldc * 4);
#pragma unroll
          for (int t = 0; t < NT; ++t) {
            float v = acc[t][i] + bv[t];
            if (act == 1) v = v > 0.f ? v : 0.f;
            if constexpr (HAS_RES) v += res[t][i];
            q[32 * t] = v;
          }
        }
      }
    };
    if (full) finish(std::false_type{});
    else finish(std::true_type{});
    arrived();
    if (!more) break;
#pragma unroll
    for (int hf = 0; hf < KH; ++hf) slab_turn(lds, lane, nx[hf], a[hf]);
    s = sn;
  }
}

// dW[64, 64] = g^T x and db = column sums of g over hundreds of thousands of rows, in the slab form of the kernel above:
// a wavefront fetches 32-row slabs of g and x as fully coalesced 1 KB requests (the next slab's are in flight under the
// current one's MFMAs), parks them in its own 2 x 8.5 KB of LDS and feeds v_mfma_f32_32x32x2_f32 from there --
// A[i][kk] = g[r + kk][32 qi + i], B[kk][j] = x[r + kk][32 qj + j], 16 steps x 4 quadrants per slab -- so every byte of g
// and x is requested from memory exactly once (tall_dw_kernel's four quadrant wavefronts each read a half of both: twice
// the L1 traffic, dword requests; 3.5 TB/s).  The four wavefronts' sums meet in LDS in a fixed order; one [64, 64] (+ [64])
// partial per workgroup goes to splitk_reduce_kernel.
// SCALED: row r of g counts row_scale[r] times (dW = (diag(s) g)^T x, db likewise): the `* ~timeline_mask` of a SASRec block
// in the backward, without a pass that writes the scaled gradient (rbx_linear_dwdb_scaled).
template <bool SCALED>
__global__ __launch_bounds__(64 * kSlabWaves, 2) void tall_dw64_kernel(const float* __restrict__ g, const long long ldg,
                                                                      const float* __restrict__ x, const long long ldx,
                                                                      const int M, float* __restrict__ dw_part,
                                                                      float* __restrict__ db_part, const int abl,
                                                                      const float* __restrict__ row_scale) {
  __shared__ float lds[kSlabWaves * 2 * 32 * kSlabLd];
  __shared__ float cs_lds[kSlabWaves][64];
  static_assert(kSlabWaves * 2 * 32 * kSlabLd >= kSlabWaves * 64 * 64, "the slabs' LDS also holds the wavefronts' [64, 64] sums");
  const int lane = threadIdx.x & 63, m = lane & 31, h = lane >> 5;
  const int wid = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  const int nw = static_cast<int>(gridDim.x) * kSlabWaves;
  const int slabs = (M + 31) >> 5;
  float* sg = lds + wid * 2 * 32 * kSlabLd;
  float* sx = sg + 32 * kSlabLd;
  f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[a][b][i] = 0.f;
  f32x4 cs = {0.f, 0.f, 0.f, 0.f};
  float* pg = sg + (lane >> 4) * kSlabLd + 4 * (lane & 15);
  float* px = sx + (lane >> 4) * kSlabLd + 4 * (lane & 15);
  // coalesced registers -> LDS (rows beyond M carry zeros in g: their products and column sums vanish)
  auto park = [&](int left, const f32x4 (&vg)[8], const f32x4 (&vx)[8], const float (&sc)[8]) {
#pragma unroll
    for (int p = 0; p < 8; ++p) {
      f32x4 u = vg[p];
      if constexpr (SCALED) u *= sc[p];
      if (left < 32 && 4 * p + (lane >> 4) >= left) u = f32x4{0.f, 0.f, 0.f, 0.f};
      cs += u;
      *reinterpret_cast<f32x4*>(pg + 4 * p * kSlabLd) = u;
      *reinterpret_cast<f32x4*>(px + 4 * p * kSlabLd) = vx[p];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  };
  int s = static_cast<int>(blockIdx.x) * kSlabWaves + wid;
  if (s < slabs) {
    unsigned og_full[8], ox_full[8], og[8], ox[8];
    slab_offsets(ldg, 32, lane, og_full);
    slab_offsets(ldx, 32, lane, ox_full);
    auto issue = [&](int sl, f32x4 (&vg)[8], f32x4 (&vx)[8], float (&sc)[8]) {
      const int left = M - sl * 32;
      if constexpr (SCALED) {                 // (plain loads in front of the slab's: they are back long before the wait below)
#pragma unroll
        for (int p = 0; p < 8; ++p) {
          const int row = sl * 32 + 4 * p + (lane >> 4);
          sc[p] = row_scale[row < M ? row : M - 1];
        }
      }
#pragma unroll
      for (int p = 0; p < 8; ++p) { og[p] = og_full[p]; ox[p] = ox_full[p]; }
      if (left < 32) {
        slab_offsets(ldg, left, lane, og);
        slab_offsets(ldx, left, lane, ox);
      }
      slab_issue(g + static_cast<long long>(sl) * 32 * ldg, og, vg);
      slab_issue(x + static_cast<long long>(sl) * 32 * ldx, ox, vx);
    };
    f32x4 ng[8], nx[8];
    float nsc[8] = {1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f};
    issue(s, ng, nx, nsc);
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(ng[0]), "+v"(ng[1]), "+v"(ng[2]), "+v"(ng[3]), "+v"(ng[4]), "+v"(ng[5]),
                 "+v"(ng[6]), "+v"(ng[7]) : : "memory");
    slab_arrived(nx);
    park(M - s * 32, ng, nx, nsc);
    const float* rg = sg + h * kSlabLd + m;
    const float* rx = sx + h * kSlabLd + m;
    for (;;) {
      int sn = s + nw;
      const bool more = sn < slabs;
      sn = more ? sn : s;
      issue(sn, ng, nx, nsc);
      if (abl != 1)
#pragma unroll
      for (int jj = 0; jj < 16; ++jj) {
        const float a0 = rg[2 * jj * kSlabLd], a1 = rg[2 * jj * kSlabLd + 32];
        const float b0 = rx[2 * jj * kSlabLd], b1 = rx[2 * jj * kSlabLd + 32];
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
      }
      asm volatile("s_waitcnt vmcnt(0)" : "+v"(ng[0]), "+v"(ng[1]), "+v"(ng[2]), "+v"(ng[3]), "+v"(ng[4]), "+v"(ng[5]),
                   "+v"(ng[6]), "+v"(ng[7]) : : "memory");
      slab_arrived(nx);
      if (!more) break;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();       // every lane has read the current slab
      s = sn;
      if (abl != 2) park(M - s * 32, ng, nx, nsc);
    }
  }
  __syncthreads();                            // all slabs consumed: the LDS now takes the four [64, 64] sums
  float* mine = lds + wid * 64 * 64;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int i = 0; i < 16; ++i) mine[(32 * a + slab_row(i) + 4 * h) * 64 + 32 * b + m] = acc[a][b][i];
  // column sums: lanes l, l ^ 16, l ^ 32, l ^ 48 hold the same four columns of different rows
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    float t = cs[c];
    t += __shfl_xor(t, 16, 64);
    t += __shfl_xor(t, 32, 64);
    if (lane < 16) cs_lds[wid][4 * lane + c] = t;
  }
  __syncthreads();
  float* out = dw_part + static_cast<long long>(blockIdx.x) * 64 * 64;
  for (int e = threadIdx.x; e < 64 * 64; e += 64 * kSlabWaves) {
    float t = lds[e];
#pragma unroll
    for (int w = 1; w < kSlabWaves; ++w) t += lds[w * 64 * 64 + e];
    out[e] = t;
  }
  if (db_part != nullptr && threadIdx.x < 64) {
    float t = cs_lds[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < kSlabWaves; ++w) t += cs_lds[w][threadIdx.x];
    db_part[static_cast<long long>(blockIdx.x) * 64 + threadIdx.x] = t;
  }
}

}  // namespace rbx
