// rbx_din.hip -- SURVEY f-4: DIN's local activation unit (gfx950).  Two ops, forward and backward each:
//
//   pairs   y[b L + l, :] = act([t_b, h_bl, t_b - h_bl, t_b o h_bl] W^T + bias)      (target_attention.py:48-53, the first
//           Linear of the attention MLP; rechub's ActivationUnit the same).  The [B L, 4E] operand is never in HBM: the
//           kernels read h [B, L, E] and t [B, E] and form the four column blocks on the way into the fp32 MFMA
//           (v_mfma_f32_32x32x2_f32: exact fp32 products and accumulation, as gemm_f32_kernel).
//   pool    w = score o mask | softmax_l(score o mask - 1e9 (1 - mask));  out[b] = sum_l w[b, l] h[b, l, :]
//           (target_attention.py:56-66).
//
// Layout: h rows of a sample are contiguous (E floats apart), samples `hist_stride_b` floats apart; t rows
// `target_stride_b` apart -- slices of rechub's [B, n_hist, L, E] block are read in place.  Everything written (y, the
// gradients, the weights) is contiguous.
//
// din_pairs_fwd_kernel   128 rows of M = B L per workgroup, a wavefront owns 32 rows x 32 NT columns.  E is walked in slices
//                        of 16: h and t[sample of the row] go k-major into a double-buffered LDS ring with the four
//                        [16, n] slices of W; the A operand of block a / b / c / d is t, h, t - h, t h computed from the two
//                        LDS reads.  The sample of a row is per ROW (a tile straddles samples whenever 128 % L != 0).
// din_pairs_dx_kernel    dP = dy' W is formed 32 columns of E at a time, as four accumulators (blocks a..d), and consumed in
//                        registers: dh = dP_b - dP_c + dP_d o t;  dt = sum_l (dP_a + dP_c + dP_d o h).  A workgroup owns
//                        WHOLE samples (128 / L of them, or one sample in chunks of 128 rows), so dt's sum over l is a loop of
//                        one thread over an LDS column: a fixed order, no atomics.
// din_pairs_dw_kernel    dW = dy'^T [t, h, t - h, t h] over a split of 1024 rows x 32 columns of E per workgroup (wavefront
//                        = block a..d), partial sums to the workspace; din_reduce_kernel adds the splits in order.  db = the
//                        column sums of dy' ride along.
// din_pool_*_kernel      one workgroup per sample; h is read once in each direction.
#include "rbx_internal.h"

namespace rbx {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kDinBM = 128;               // rows per tile
constexpr int kDinKC = 16;                // columns of E per k step of the forward
constexpr int kDinLdA = kDinBM + 2;       // LDS pitch of a k row of a [k, 128 rows] operand (conflict-free transposed stores)
constexpr int kDinMaxN = 64, kDinMinDim = 4, kDinMaxDim = 128;
constexpr int kDinEC = 32;                // columns of E per pass of the backward kernels
constexpr int kDinDwRows = 1024;          // rows per split of the dW reduction
constexpr int kDinDwStep = 32;            // rows per k step of the dW kernel
constexpr int kDinPoolMaxL = 4096;        // the pool kernels keep one float per position in LDS

// C/D layout of the 32 x 32 MFMA: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
__device__ __forceinline__ int din_acc_row(int r, int lk) { return (r & 3) + 8 * (r >> 2) + 4 * lk; }

__device__ __forceinline__ float4 din_ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// ---- pairs forward ----------------------------------------------------------------------------------------------------
// dynamic LDS: Hs 2 x [16][130] | Ts 2 x [16][130] | Ws 2 x [4 blocks][16][32 NT + 2]
template <int NT>
__global__ __launch_bounds__(256) void din_pairs_fwd_kernel(const float* __restrict__ H, const long long hist_stride,
                                                            const float* __restrict__ T, const long long target_stride,
                                                            const int M, const int L, const int E,
                                                            const float* __restrict__ W, const float* __restrict__ bias,
                                                            const int n, const int act, float* __restrict__ Y) {
  constexpr int NP = 32 * NT, LDW = NP + 2;
  extern __shared__ float smem[];
  float* Hs = smem;
  float* Ts = Hs + 2 * kDinKC * kDinLdA;
  float* Ws = Ts + 2 * kDinKC * kDinLdA;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, li = lane & 31, lk = lane >> 5;
  const int row0 = static_cast<int>(blockIdx.x) * kDinBM;

  // this thread's two (row, 4 columns) pieces of every [128, 16] slice of h and t
  const float* hp[2];
  const float* tp[2];
  const int k4 = (tid & 3) * 4;
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int row = row0 + (tid >> 2) + 64 * p;
    hp[p] = nullptr;
    tp[p] = nullptr;
    if (row < M) {
      const int b = row / L, l = row - b * L;
      hp[p] = H + b * hist_stride + static_cast<long long>(l) * E + k4;
      tp[p] = T + b * target_stride + k4;
    }
  }
  float4 hreg[2], treg[2], wreg[2 * NT];
  auto load = [&](const int e0) {
    const bool in = e0 + k4 < E;                 // E % 4 == 0: a float4 is inside or outside as a whole
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const bool ok = in && hp[p] != nullptr;
      hreg[p] = ok ? din_ld4(hp[p] + e0) : make_float4(0.f, 0.f, 0.f, 0.f);
      treg[p] = ok ? din_ld4(tp[p] + e0) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int p = 0; p < 2 * NT; ++p) {
      const int i = tid + 256 * p, nn = (i >> 2) % NP, blk = (i >> 2) / NP;
      wreg[p] = (in && nn < n) ? din_ld4(W + static_cast<long long>(nn) * 4 * E + blk * E + e0 + k4)
                               : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  auto store = [&](const int buf) {
    float* hs = Hs + buf * kDinKC * kDinLdA;
    float* ts = Ts + buf * kDinKC * kDinLdA;
    float* ws = Ws + buf * 4 * kDinKC * LDW;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int r = (tid >> 2) + 64 * p;
      hs[(k4 + 0) * kDinLdA + r] = hreg[p].x; hs[(k4 + 1) * kDinLdA + r] = hreg[p].y;
      hs[(k4 + 2) * kDinLdA + r] = hreg[p].z; hs[(k4 + 3) * kDinLdA + r] = hreg[p].w;
      ts[(k4 + 0) * kDinLdA + r] = treg[p].x; ts[(k4 + 1) * kDinLdA + r] = treg[p].y;
      ts[(k4 + 2) * kDinLdA + r] = treg[p].z; ts[(k4 + 3) * kDinLdA + r] = treg[p].w;
    }
#pragma unroll
    for (int p = 0; p < 2 * NT; ++p) {
      const int i = tid + 256 * p, nn = (i >> 2) % NP, blk = (i >> 2) / NP;
      float* dst = ws + (blk * kDinKC + k4) * LDW + nn;
      dst[0] = wreg[p].x; dst[LDW] = wreg[p].y; dst[2 * LDW] = wreg[p].z; dst[3 * LDW] = wreg[p].w;
    }
  };

  f32x16 acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

  const int steps = (E + kDinKC - 1) / kDinKC;
  load(0);
  store(0);
  __syncthreads();
  int cur = 0;
  for (int c = 0; c < steps; ++c) {
    const bool more = c + 1 < steps;
    if (more) load((c + 1) * kDinKC);            // flies under the MFMAs
    const float* hs = Hs + cur * kDinKC * kDinLdA + wv * 32 + li;
    const float* ts = Ts + cur * kDinKC * kDinLdA + wv * 32 + li;
    const float* ws = Ws + cur * 4 * kDinKC * LDW + li;
#pragma unroll
    for (int kk = 0; kk < kDinKC; kk += 2) {
      const float hv = hs[(kk + lk) * kDinLdA], tv = ts[(kk + lk) * kDinLdA];
      const float a[4] = {tv, hv, tv - hv, tv * hv};
#pragma unroll
      for (int blk = 0; blk < 4; ++blk)
#pragma unroll
        for (int j = 0; j < NT; ++j)
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[blk], ws[(blk * kDinKC + kk + lk) * LDW + j * 32], acc[j], 0, 0, 0);
    }
    if (more) store(cur ^ 1);
    __syncthreads();
    cur ^= 1;
  }

#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int col = j * 32 + li;
    if (col >= n) continue;
    const float bv = bias != nullptr ? bias[col] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = row0 + wv * 32 + din_acc_row(r, lk);
      if (row < M) {
        float v = acc[j][r] + bv;
        if (act != 0) v = v < 0.f ? 0.f : v;
        Y[static_cast<long long>(row) * n + col] = v;
      }
    }
  }
}

// ---- pairs backward: dh, dt -------------------------------------------------------------------------------------------
// dynamic LDS: dys [64 k = unit][130] (dy' of the tile, k-major, zero beyond n) | Ws [4 blocks][64 units][32], re-used as
// the [128 rows][33] dt contributions of the pass
__global__ __launch_bounds__(256) void din_pairs_dx_kernel(const float* __restrict__ H, const long long hist_stride,
                                                           const float* __restrict__ T, const long long target_stride,
                                                           const int B, const int L, const int E,
                                                           const float* __restrict__ W, const int n, const int act,
                                                           const float* __restrict__ Y, const float* __restrict__ dY,
                                                           float* __restrict__ dH, float* __restrict__ dT, const int S) {
  extern __shared__ float smem[];
  __shared__ int s_b[kDinBM];
  float* dys = smem;
  float* Ws = dys + kDinMaxN * kDinLdA;
  float* cs = Ws;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, li = lane & 31, lk = lane >> 5;
  const int b_first = static_cast<int>(blockIdx.x) * S;
  const int b_last = b_first + S < B ? b_first + S : B;
  const int g_begin = b_first * L, g_end = b_last * L;     // the rows of M = B L this workgroup owns: whole samples
  const int kend = (n + 1) & ~1;

  for (int row0 = g_begin; row0 < g_end; row0 += kDinBM) {
    const int nrows = g_end - row0 < kDinBM ? g_end - row0 : kDinBM;
    __syncthreads();                                         // the previous chunk's readers of dys / cs / s_b are done
    for (int i = tid; i < kDinBM * kDinMaxN; i += 256) {
      const int r = i / kDinMaxN, c = i % kDinMaxN;
      float v = 0.f;
      if (r < nrows && c < n) {
        const long long at = static_cast<long long>(row0 + r) * n + c;
        v = dY[at];
        if (act != 0 && !(Y[at] > 0.f)) v = 0.f;
      }
      dys[c * kDinLdA + r] = v;
    }
    if (tid < kDinBM) s_b[tid] = tid < nrows ? (row0 + tid) / L : 0;
    const int b0 = row0 / L;
    const int ns = (row0 + nrows - 1) / L - b0 + 1;          // samples with rows in this chunk

    for (int e0 = 0; e0 < E; e0 += kDinEC) {
      __syncthreads();                                       // dys is written; the previous pass is done with cs
      for (int i = tid; i < 4 * kDinMaxN * (kDinEC / 4); i += 256) {
        const int c4 = (i & 7) * 4, nn = (i >> 3) % kDinMaxN, blk = (i >> 3) / kDinMaxN;
        const float4 v = (nn < n && e0 + c4 < E) ? din_ld4(W + static_cast<long long>(nn) * 4 * E + blk * E + e0 + c4)
                                                 : make_float4(0.f, 0.f, 0.f, 0.f);
        *reinterpret_cast<float4*>(Ws + (blk * kDinMaxN + nn) * kDinEC + c4) = v;
      }
      __syncthreads();
      f32x16 acc[4];
#pragma unroll
      for (int blk = 0; blk < 4; ++blk)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[blk][r] = 0.f;
      for (int kk = 0; kk < kend; kk += 2) {
        const float a = dys[(kk + lk) * kDinLdA + wv * 32 + li];
#pragma unroll
        for (int blk = 0; blk < 4; ++blk)
          acc[blk] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, Ws[(blk * kDinMaxN + kk + lk) * kDinEC + li], acc[blk], 0, 0, 0);
      }
      __syncthreads();                                       // every wavefront has read Ws: cs may overwrite it
      const int col = e0 + li;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rl = wv * 32 + din_acc_row(r, lk);
        float contrib = 0.f;
        if (rl < nrows && col < E) {
          const int g = row0 + rl, b = s_b[rl], l = g - b * L;
          const float hv = H[b * hist_stride + static_cast<long long>(l) * E + col];
          const float tv = T[b * target_stride + col];
          if (dH != nullptr) dH[static_cast<long long>(g) * E + col] = acc[1][r] - acc[2][r] + acc[3][r] * tv;
          contrib = acc[0][r] + acc[2][r] + acc[3][r] * hv;
        }
        cs[rl * (kDinEC + 1) + li] = contrib;
      }
      __syncthreads();
      if (dT != nullptr) {
        for (int i = tid; i < ns * kDinEC; i += 256) {
          const int s = i >> 5, c = i & 31;
          if (e0 + c >= E) continue;
          const int first = (b0 + s) * L, last = first + L;
          const int lo = (first > row0 ? first : row0) - row0;
          const int hi = (last < row0 + nrows ? last : row0 + nrows) - row0;
          float sum = 0.f;
          for (int r = lo; r < hi; ++r) sum += cs[r * (kDinEC + 1) + c];
          float* dst = dT + static_cast<long long>(b0 + s) * E + e0 + c;
          // a sample longer than one chunk: the same thread adds its later chunks, in order
          *dst = first >= row0 ? sum : *dst + sum;
        }
      }
    }
  }
}

// ---- pairs backward: dW, db -------------------------------------------------------------------------------------------
// part [splits][n 4E + n]: the split's dW, then its db
template <int NT>
__global__ __launch_bounds__(256) void din_pairs_dw_kernel(const float* __restrict__ H, const long long hist_stride,
                                                           const float* __restrict__ T, const long long target_stride,
                                                           const int M, const int L, const int E, const int n, const int act,
                                                           const float* __restrict__ Y, const float* __restrict__ dY,
                                                           float* __restrict__ part) {
  constexpr int NP = 32 * NT;
  __shared__ float dys[2][kDinDwStep * NP];
  __shared__ __attribute__((aligned(16))) float hs[2][kDinDwStep * kDinEC];
  __shared__ __attribute__((aligned(16))) float ts[2][kDinDwStep * kDinEC];
  const int tid = threadIdx.x, lane = tid & 63, blk = tid >> 6, li = lane & 31, lk = lane >> 5;
  const int r_begin = static_cast<int>(blockIdx.x) * kDinDwRows;
  const int r_end = r_begin + kDinDwRows < M ? r_begin + kDinDwRows : M;
  const int e0 = static_cast<int>(blockIdx.y) * kDinEC;
  const bool with_db = blockIdx.y == 0 && tid < n;

  float dreg[4 * NT];
  float4 hreg, treg;
  auto load = [&](const int row0) {
#pragma unroll
    for (int p = 0; p < 4 * NT; ++p) {
      const int i = tid + 256 * p, r = row0 + i / NP, c = i % NP;
      float v = 0.f;
      if (r < r_end && c < n) {
        const long long at = static_cast<long long>(r) * n + c;
        v = dY[at];
        if (act != 0 && !(Y[at] > 0.f)) v = 0.f;
      }
      dreg[p] = v;
    }
    const int r = row0 + (tid >> 3), c4 = e0 + (tid & 7) * 4;
    hreg = make_float4(0.f, 0.f, 0.f, 0.f);
    treg = hreg;
    if (r < r_end && c4 < E) {
      const int b = r / L, l = r - b * L;
      hreg = din_ld4(H + b * hist_stride + static_cast<long long>(l) * E + c4);
      treg = din_ld4(T + b * target_stride + c4);
    }
  };
  auto store = [&](const int buf) {
#pragma unroll
    for (int p = 0; p < 4 * NT; ++p) dys[buf][tid + 256 * p] = dreg[p];
    *reinterpret_cast<float4*>(&hs[buf][tid * 4]) = hreg;
    *reinterpret_cast<float4*>(&ts[buf][tid * 4]) = treg;
  };

  f32x16 acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
  float dbsum = 0.f;

  load(r_begin);
  store(0);
  __syncthreads();
  int cur = 0;
  for (int row0 = r_begin; row0 < r_end; row0 += kDinDwStep) {
    const bool more = row0 + kDinDwStep < r_end;
    if (more) load(row0 + kDinDwStep);
#pragma unroll
    for (int kk = 0; kk < kDinDwStep; kk += 2) {
      const float hv = hs[cur][(kk + lk) * kDinEC + li], tv = ts[cur][(kk + lk) * kDinEC + li];
      const float bv = blk == 0 ? tv : (blk == 1 ? hv : (blk == 2 ? tv - hv : tv * hv));
#pragma unroll
      for (int j = 0; j < NT; ++j)
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(dys[cur][(kk + lk) * NP + j * 32 + li], bv, acc[j], 0, 0, 0);
    }
    if (with_db)
      for (int k = 0; k < kDinDwStep; ++k) dbsum += dys[cur][k * NP + tid];
    if (more) store(cur ^ 1);
    __syncthreads();
    cur ^= 1;
  }

  float* mine = part + static_cast<long long>(blockIdx.x) * (static_cast<long long>(n) * 4 * E + n);
  const int col = e0 + li;
  if (col < E) {
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int nn = j * 32 + din_acc_row(r, lk);
        if (nn < n) mine[static_cast<long long>(nn) * 4 * E + blk * E + col] = acc[j][r];
      }
  }
  if (with_db) mine[static_cast<long long>(n) * 4 * E + tid] = dbsum;
}

__global__ __launch_bounds__(256) void din_reduce_kernel(const float* __restrict__ part, const int splits, const int n_dw,
                                                         const int n_db, float* __restrict__ dW, float* __restrict__ db) {
  const int j = static_cast<int>(blockIdx.x) * 256 + threadIdx.x, total = n_dw + n_db;
  if (j >= total) return;
  float sum = 0.f;
  for (int s = 0; s < splits; ++s) sum += part[static_cast<long long>(s) * total + j];
  if (j < n_dw) {
    if (dW != nullptr) dW[j] = sum;
  } else if (db != nullptr) {
    db[j - n_dw] = sum;
  }
}

// ---- pool -------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float din_block_sum(float v, float* red) {
  v = group_sum<64>(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const float r = (red[0] + red[1]) + (red[2] + red[3]);
  __syncthreads();
  return r;
}
__device__ __forceinline__ float din_block_max(float v, float* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const float r = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(256) void din_pool_fwd_kernel(const float* __restrict__ score, const float* __restrict__ mask,
                                                           const float* __restrict__ H, const long long hist_stride,
                                                           const int L, const int E, const int softmax,
                                                           float* __restrict__ weight, float* __restrict__ out) {
  __shared__ float s_w[kDinPoolMaxL];
  __shared__ __attribute__((aligned(16))) float s_part[8][kDinMaxDim];
  __shared__ float s_red[4];
  const int tid = threadIdx.x;
  const long long b = blockIdx.x;
  const float* sc = score + b * L;
  const float* mk = mask != nullptr ? mask + b * L : nullptr;
  float* wt = weight + b * L;
  if (softmax != 0) {
    float mx = -INFINITY;
    for (int l = tid; l < L; l += 256) {
      float x = sc[l];
      if (mk != nullptr) x = x * mk[l] + -1.0e9f * (1.f - mk[l]);
      s_w[l] = x;
      mx = fmaxf(mx, x);
    }
    mx = din_block_max(mx, s_red);
    float sum = 0.f;
    for (int l = tid; l < L; l += 256) {
      const float e = expf(s_w[l] - mx);
      s_w[l] = e;
      sum += e;
    }
    sum = din_block_sum(sum, s_red);
    for (int l = tid; l < L; l += 256) {
      const float w = s_w[l] / sum;
      s_w[l] = w;
      wt[l] = w;
    }
  } else {
    for (int l = tid; l < L; l += 256) {
      const float w = mk != nullptr ? sc[l] * mk[l] : sc[l];
      s_w[l] = w;
      wt[l] = w;
    }
  }
  __syncthreads();
  const int g = tid >> 5, c4 = (tid & 31) * 4;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (c4 < E) {
    const float* h = H + b * hist_stride + c4;
    for (int l = g; l < L; l += 8) {
      const float4 v = din_ld4(h + static_cast<long long>(l) * E);
      const float w = s_w[l];
      acc.x += w * v.x; acc.y += w * v.y; acc.z += w * v.z; acc.w += w * v.w;
    }
  }
  *reinterpret_cast<float4*>(&s_part[g][c4]) = acc;
  __syncthreads();
  if (tid < E) {
    float sum = 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) sum += s_part[q][tid];
    out[b * E + tid] = sum;
  }
}

__global__ __launch_bounds__(256) void din_pool_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ weight,
                                                           const float* __restrict__ mask, const float* __restrict__ H,
                                                           const long long hist_stride, const int L, const int E,
                                                           const int softmax, float* __restrict__ dscore,
                                                           float* __restrict__ dH) {
  __shared__ float s_dw[kDinPoolMaxL];
  __shared__ __attribute__((aligned(16))) float s_do[kDinMaxDim];
  __shared__ float s_red[4];
  const int tid = threadIdx.x;
  const long long b = blockIdx.x;
  const float* wt = weight + b * L;
  if (tid < E) s_do[tid] = dout[b * E + tid];
  __syncthreads();
  // dw[l] = <dout, h_l>: 8 lanes per row, 32 rows per round
  const int sub = tid & 7, rg = tid >> 3;
  const float* h = H + b * hist_stride;
  for (int l0 = 0; l0 < L; l0 += 32) {
    const int l = l0 + rg;
    float p = 0.f;
    if (l < L)
      for (int c4 = sub * 4; c4 < E; c4 += 32) {
        const float4 v = din_ld4(h + static_cast<long long>(l) * E + c4);
        const float4 d = *reinterpret_cast<const float4*>(&s_do[c4]);
        p += v.x * d.x + v.y * d.y + v.z * d.z + v.w * d.w;
      }
    p = group_sum<8>(p);
    if (l < L && sub == 0) s_dw[l] = p;
  }
  __syncthreads();
  if (dscore != nullptr) {
    float dot = 0.f;
    if (softmax != 0) {
      for (int l = tid; l < L; l += 256) dot += wt[l] * s_dw[l];
      dot = din_block_sum(dot, s_red);
    }
    for (int l = tid; l < L; l += 256) {
      float d = softmax != 0 ? wt[l] * (s_dw[l] - dot) : s_dw[l];
      if (mask != nullptr) d *= mask[b * L + l];
      dscore[b * L + l] = d;
    }
  }
  if (dH != nullptr) {
    const int e4 = E / 4;
    float* dst = dH + b * L * E;
    for (int i = tid; i < L * e4; i += 256) {
      const int l = i / e4, c4 = (i - l * e4) * 4;
      const float w = wt[l];
      const float4 d = *reinterpret_cast<const float4*>(&s_do[c4]);
      *reinterpret_cast<float4*>(dst + static_cast<long long>(l) * E + c4) = make_float4(w * d.x, w * d.y, w * d.z, w * d.w);
    }
  }
}

// ---- host -------------------------------------------------------------------------------------------------------------
static int din_splits(long long m) { return static_cast<int>((m + kDinDwRows - 1) / kDinDwRows); }

// RBX_OK, or the refusal of a shape none of the kernels serves
static int din_check_shape(const char* what, int64_t batch, int32_t seq_len, int32_t dim) {
  if (batch < 0) return fail(RBX_ERR_INVALID, "%s: batch=%lld", what, static_cast<long long>(batch));
  if (dim < kDinMinDim || dim > kDinMaxDim || (dim & 3) != 0)
    return fail(RBX_ERR_UNSUPPORTED, "%s: dim=%d is not a multiple of 4 in [%d,%d]", what, dim, kDinMinDim, kDinMaxDim);
  if (seq_len < 1) return fail(RBX_ERR_UNSUPPORTED, "%s: seq_len=%d", what, seq_len);
  if (batch * static_cast<long long>(seq_len) > INT_MAX)
    return fail(RBX_ERR_UNSUPPORTED, "%s: batch * seq_len = %lld does not fit an int32", what,
                static_cast<long long>(batch) * seq_len);
  return RBX_OK;
}

static int din_check_operands(const char* what, const float* hist, int64_t hist_stride, const float* target,
                              int64_t target_stride) {
  if (!aligned16(hist) || (hist_stride & 3) != 0 || (target != nullptr && (!aligned16(target) || (target_stride & 3) != 0)))
    return fail(RBX_ERR_UNSUPPORTED, "%s: bases must be 16-byte aligned and sample strides multiples of 4 floats", what);
  return RBX_OK;
}

template <int NT>
static int din_launch_fwd(const float* H, long long hs, const float* T, long long ts, int M, int L, int E, const float* W,
                          const float* bias, int n, int act, float* Y, hipStream_t s) {
  const size_t lds = (4 * kDinKC * kDinLdA + 2 * 4 * kDinKC * (32 * NT + 2)) * sizeof(float);
  const int rc = allow_lds("din_pairs_fwd", &din_pairs_fwd_kernel<NT>, lds);
  if (rc != RBX_OK) return rc;
  hipLaunchKernelGGL((din_pairs_fwd_kernel<NT>), dim3((M + kDinBM - 1) / kDinBM), dim3(256), lds, s, H, hs, T, ts, M, L, E, W,
                     bias, n, act, Y);
  return RBX_OK;
}

}  // namespace rbx

extern "C" int rbx_din_pairs_fwd(const float* d_hist, int64_t hist_stride_b, const float* d_target, int64_t target_stride_b,
                                 int64_t batch, int32_t seq_len, int32_t dim, const float* d_w, const float* d_bias,
                                 int32_t n, int32_t act, float* d_y, void* stream) {
  using namespace rbx;
  int rc = din_check_shape("din_pairs_fwd", batch, seq_len, dim);
  if (rc != RBX_OK) return rc;
  if (n < 1 || n > kDinMaxN) return fail(RBX_ERR_UNSUPPORTED, "din_pairs_fwd: n=%d not in [1,%d]", n, kDinMaxN);
  if (act != 0 && act != 1) return fail(RBX_ERR_UNSUPPORTED, "din_pairs_fwd: act=%d", act);
  if (batch == 0) return RBX_OK;
  if (!d_hist || !d_target || !d_w || !d_y) return fail(RBX_ERR_INVALID, "din_pairs_fwd: NULL tensor");
  rc = din_check_operands("din_pairs_fwd", d_hist, hist_stride_b, d_target, target_stride_b);
  if (rc != RBX_OK) return rc;
  if (!aligned16(d_w)) return fail(RBX_ERR_UNSUPPORTED, "din_pairs_fwd: the weight must be 16-byte aligned");
  const int M = static_cast<int>(batch * seq_len);
  hipStream_t s = as_stream(stream);
  rc = n > 32 ? din_launch_fwd<2>(d_hist, hist_stride_b, d_target, target_stride_b, M, seq_len, dim, d_w, d_bias, n, act, d_y, s)
              : din_launch_fwd<1>(d_hist, hist_stride_b, d_target, target_stride_b, M, seq_len, dim, d_w, d_bias, n, act, d_y, s);
  if (rc != RBX_OK) return rc;
  return check_launch("din_pairs_fwd");
}

extern "C" size_t rbx_din_pairs_bwd_workspace_size(int64_t batch, int32_t seq_len, int32_t dim, int32_t n) {
  using namespace rbx;
  if (batch <= 0 || seq_len < 1 || dim < kDinMinDim || dim > kDinMaxDim || n < 1 || n > kDinMaxN) return 0;
  if (batch * static_cast<long long>(seq_len) > INT_MAX) return 0;
  const size_t per = (static_cast<size_t>(n) * 4 * dim + n) * sizeof(float);
  return (din_splits(batch * static_cast<long long>(seq_len)) * per + 255) / 256 * 256;
}

extern "C" int rbx_din_pairs_bwd(const float* d_hist, int64_t hist_stride_b, const float* d_target, int64_t target_stride_b,
                                 int64_t batch, int32_t seq_len, int32_t dim, const float* d_w, int32_t n, int32_t act,
                                 const float* d_y, const float* d_dy, float* d_dhist, float* d_dtarget, float* d_dw,
                                 float* d_db, void* d_workspace, size_t workspace_bytes, void* stream) {
  using namespace rbx;
  int rc = din_check_shape("din_pairs_bwd", batch, seq_len, dim);
  if (rc != RBX_OK) return rc;
  if (n < 1 || n > kDinMaxN) return fail(RBX_ERR_UNSUPPORTED, "din_pairs_bwd: n=%d not in [1,%d]", n, kDinMaxN);
  if (act != 0 && act != 1) return fail(RBX_ERR_UNSUPPORTED, "din_pairs_bwd: act=%d", act);
  if (batch == 0) return RBX_OK;
  if (!d_hist || !d_target || !d_w || !d_dy || (act != 0 && !d_y)) return fail(RBX_ERR_INVALID, "din_pairs_bwd: NULL tensor");
  rc = din_check_operands("din_pairs_bwd", d_hist, hist_stride_b, d_target, target_stride_b);
  if (rc != RBX_OK) return rc;
  if (!aligned16(d_w) || (d_dhist != nullptr && !aligned16(d_dhist)))
    return fail(RBX_ERR_UNSUPPORTED, "din_pairs_bwd: the weight and dhist must be 16-byte aligned");
  const bool want_w = d_dw != nullptr || d_db != nullptr;
  if (want_w && (d_workspace == nullptr || workspace_bytes < rbx_din_pairs_bwd_workspace_size(batch, seq_len, dim, n)))
    return fail(RBX_ERR_WORKSPACE, "din_pairs_bwd: workspace too small");
  const int M = static_cast<int>(batch * seq_len), B = static_cast<int>(batch);
  hipStream_t s = as_stream(stream);
  if (d_dhist != nullptr || d_dtarget != nullptr) {
    const int S = seq_len >= kDinBM ? 1 : kDinBM / seq_len;
    const size_t lds = (kDinMaxN * kDinLdA + 4 * kDinMaxN * kDinEC) * sizeof(float);
    rc = allow_lds("din_pairs_bwd", &din_pairs_dx_kernel, lds);
    if (rc != RBX_OK) return rc;
    hipLaunchKernelGGL(din_pairs_dx_kernel, dim3((B + S - 1) / S), dim3(256), lds, s, d_hist, hist_stride_b, d_target,
                       target_stride_b, B, seq_len, dim, d_w, n, act, d_y, d_dy, d_dhist, d_dtarget, S);
  }
  if (want_w) {
    const int splits = din_splits(M);
    float* part = static_cast<float*>(d_workspace);
    const dim3 grid(splits, (dim + kDinEC - 1) / kDinEC);
    if (n > 32)
      hipLaunchKernelGGL((din_pairs_dw_kernel<2>), grid, dim3(256), 0, s, d_hist, hist_stride_b, d_target, target_stride_b, M,
                         seq_len, dim, n, act, d_y, d_dy, part);
    else
      hipLaunchKernelGGL((din_pairs_dw_kernel<1>), grid, dim3(256), 0, s, d_hist, hist_stride_b, d_target, target_stride_b, M,
                         seq_len, dim, n, act, d_y, d_dy, part);
    const int n_dw = n * 4 * dim;
    hipLaunchKernelGGL(din_reduce_kernel, dim3((n_dw + n + 255) / 256), dim3(256), 0, s, part, splits, n_dw, n, d_dw, d_db);
  }
  return check_launch("din_pairs_bwd");
}

extern "C" int rbx_din_pool_fwd(const float* d_score, const float* d_mask, const float* d_hist, int64_t hist_stride_b,
                                int64_t batch, int32_t seq_len, int32_t dim, int32_t softmax, float* d_weight, float* d_out,
                                void* stream) {
  using namespace rbx;
  int rc = din_check_shape("din_pool_fwd", batch, seq_len, dim);
  if (rc != RBX_OK) return rc;
  if (seq_len > kDinPoolMaxL) return fail(RBX_ERR_UNSUPPORTED, "din_pool_fwd: seq_len=%d above %d", seq_len, kDinPoolMaxL);
  if (batch == 0) return RBX_OK;
  if (!d_score || !d_hist || !d_weight || !d_out) return fail(RBX_ERR_INVALID, "din_pool_fwd: NULL tensor");
  rc = din_check_operands("din_pool_fwd", d_hist, hist_stride_b, nullptr, 0);
  if (rc != RBX_OK) return rc;
  hipLaunchKernelGGL(din_pool_fwd_kernel, dim3(static_cast<unsigned>(batch)), dim3(256), 0, as_stream(stream), d_score, d_mask,
                     d_hist, hist_stride_b, seq_len, dim, softmax, d_weight, d_out);
  return check_launch("din_pool_fwd");
}

extern "C" int rbx_din_pool_bwd(const float* d_dout, const float* d_weight, const float* d_mask, const float* d_hist,
                                int64_t hist_stride_b, int64_t batch, int32_t seq_len, int32_t dim, int32_t softmax,
                                float* d_dscore, float* d_dhist, void* stream) {
  using namespace rbx;
  int rc = din_check_shape("din_pool_bwd", batch, seq_len, dim);
  if (rc != RBX_OK) return rc;
  if (seq_len > kDinPoolMaxL) return fail(RBX_ERR_UNSUPPORTED, "din_pool_bwd: seq_len=%d above %d", seq_len, kDinPoolMaxL);
  if (batch == 0) return RBX_OK;
  if (!d_dout || !d_weight || !d_hist) return fail(RBX_ERR_INVALID, "din_pool_bwd: NULL tensor");
  rc = din_check_operands("din_pool_bwd", d_hist, hist_stride_b, nullptr, 0);
  if (rc != RBX_OK) return rc;
  if (d_dhist != nullptr && !aligned16(d_dhist)) return fail(RBX_ERR_UNSUPPORTED, "din_pool_bwd: dhist must be 16-byte aligned");
  hipLaunchKernelGGL(din_pool_bwd_kernel, dim3(static_cast<unsigned>(batch)), dim3(256), 0, as_stream(stream), d_dout, d_weight,
                     d_mask, d_hist, hist_stride_b, seq_len, dim, softmax, d_dscore, d_dhist);
  return check_launch("din_pool_bwd");
}
