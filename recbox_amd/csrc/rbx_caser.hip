// rbx_caser.hip -- Caser's convolutional layers (gfx950, wave64): the L horizontal convolutions with their ReLU and max over time, the
// vertical convolution and both concatenations of third_party/recbole/model/sequential_recommender/caser.py:121-137 as one launch
// forward.  Replaces 3 L + 1 ATen launches (a Conv2d, a ReLU and a max_pool1d per height, one cat of the L pieces), the vertical
// Conv2d, the second cat and the [B, n_h, L - h + 1] activations autograd keeps per height.  x [B, L, D] is the embedded session,
// w_h[h - 1] [n_h, h, D], b_h[h - 1] [n_h] for h = 1 .. L, w_v [n_v, L], b_v [n_v]; out [B, n_v D + n_h L]:
//   out[b, v D + d]                 = b_v[v] + sum_l w_v[v, l] x[b, l, d]
//   out[b, n_v D + (h - 1) n_h + f] = max_{t <= L - h} relu(b_h[h - 1][f] + sum_{i < h, d} w_h[h - 1][f, i, d] x[b, t + i, d])
// No padding mask: the zero rows of padded positions are convolved like any other, as in the reference.
//
// The L weight and bias pointers travel in the kernel's argument segment (CsPtrs, 800 bytes): nothing is packed or copied.
//
// caser_fwd_kernel   a workgroup of 8 wavefronts owns a TILE of 16 samples at a time (8 where cs_lds(L, D, 16) = 4 (16 (L D + 4) +
//                    max(16 (pad4(L) + 4), 192)) bytes exceed the 160 KiB of a compute unit, that is where L D + pad4(L) > 2552:
//                    39 x 64 still takes 16; 40 x 64, 45 x 56 and 50 x 64 take 8; the upper 8 rows of the MFMA tile are then zeros) and walks the tiles blockIdx, blockIdx +
//                    grid, ...; the grid is min(tiles, 256): at 130 VGPRs a SIMD holds 3 wavefronts and a workgroup puts 2 on
//                    each, so a compute unit holds one workgroup whatever the LDS.  The tile's [L, D] blocks are
//                    staged once, a row per sample.  A window x[b, t : t + h, :] is then h D contiguous floats of that row and the
//                    n_h filters of height h are an [h D, n_h] matrix, so one (h, t) is a [16, h D] x [h D, n_h] product on
//                    v_mfma_f32_16x16x4_f32 (exact fp32).  A wavefront owns the heights wave + 1, wave + 9, ...; per height it walks
//                    the windows 8 at a time over one pass through w_h (cs_windows: one weight fetch feeds 8 MFMAs; the weights
//                    come through L1 / L2, at most n_h D L (L + 1) / 2 floats = 5.2 MiB in all) and keeps the running maximum and
//                    its first t in registers.  max_t relu(p_t + b) = relu(max_t p_t + b), so the bias and the ReLU are applied
//                    once.  It writes out and the winner t* [B, L n_h] as int8 (-1: the ReLU is shut, no gradient).  The vertical
//                    rows are [n_v, L] x [L, D] per sample on the same MFMA (mm16) from the same LDS rows, w_v staged once per
//                    workgroup.
// caser_dx_kernel    a workgroup per sample (grid min(4096, ceil(B / 2)), samples blockIdx, blockIdx + grid, ...).  The sample's
//                    live g and t* D go to LDS; a thread owns an element p of dx[b] and adds, over h and f ascending, g w_h[h - 1]
//                    [f][p - t* D] where p lies in the winning window, then over v ascending w_v[v, l] g_v[v, d]: dx stays in a
//                    register, every sum has one order.
// caser_dw_kernel    a thread owns ONE element of (dW_h | db_h | dW_v | db_v), P = n_h D L (L + 1) / 2 + n_h L + n_v L + n_v in
//                    all, and a run of samples, which it walks in ascending order: dW_h[h - 1][f, i, d] += g x[b, t* + i, d].
//                    grid = (ceil(P / 256), R): R runs of ceil(B / R) samples, R = min(32, ceil(4096 / chunks), ceil(B / 32)), so
//                    that small filter banks still fill the GPU and large ones (1.3 M elements at 50 x 64 x 16) take one run.
//                    It writes row `run` of the workspace [R][P].
// caser_tail_kernel  adds the R rows in ascending order (colsum16) into the L + L + 2 gradient tensors.
// No atomics: two runs give the same bits.  No host read-back, nothing allocated, everything on the caller's stream, no launch
// with an empty grid.  Every index is bounded by batch, L, D, n_h and n_v.
#include "rbx_internal.h"
#include "rbx_tile16.h"

namespace rbx {

constexpr int kCsMaxL = 50, kCsMaxD = 64, kCsMaxNh = 16, kCsMaxNv = 16;
constexpr int kCsTile = 16;                 // samples of a tile: the M of one MFMA
constexpr int kCsWin = 8;                   // windows that share one pass through the weights
constexpr int kCsFwdThreads = 512;
constexpr int kCsFwdPerCU = 1;              // resident workgroups of the forward per compute unit: 8 wavefronts at 3 per SIMD
constexpr int kCsFwdMaxGrid = kCUs * kCsFwdPerCU;
constexpr int kCsDxMaxGrid = 4096;
constexpr int kCsDwTarget = 4096, kCsDwMaxRuns = 32, kCsDwMinRun = 32;
constexpr size_t kCsLdsCap = 160 * 1024;    // LDS of a gfx950 compute unit

struct CsPtrs {
  const float* w[kCsMaxL];   // w_h[h - 1]: [n_h][h D]
  const float* b[kCsMaxL];   // b_h[h - 1]: [n_h]
};
struct CsOut {
  float* dw[kCsMaxL];
  float* db[kCsMaxL];
};

struct CsFwd {
  const float* x;            // [B, L, D] at strides sb, sl, 1
  const float* wv;           // [n_v, L] or NULL
  const float* bv;           // [n_v] or NULL
  float* out;                // [B, n_v D + n_h L]
  signed char* win;          // [B, L n_h] or NULL
  long long B, sb;
  int sl, L, D, nh, nv, T;
  CsPtrs h;
};

struct CsBwd {
  const float* x;
  const float* g;            // [B, n_v D + n_h L]
  const signed char* win;    // [B, L n_h]
  const float* wv;
  float* dx;                 // [B, L, D] contiguous
  float* part;               // [R][P]
  long long B, sb, run;
  int sl, L, D, nh, nv, E, P;
  CsPtrs h;
};

struct CsTail {
  const float* part;
  float* dwv;
  float* dbv;
  int R, P, E, L, D, nh, nv;
  CsOut h;
};

static __host__ __device__ inline int cs_pad4(int n) { return (n + 3) & ~3; }
static __host__ __device__ inline int cs_lda(int L, int D) { return L * D + 4; }
static __host__ __device__ inline int cs_ldv(int L) { return cs_pad4(L) + 4; }
// the staged w_v [16][pad4(L) + 4]; at least 3 D floats, which the vertical product's masked k reads behind the last sample's row
static __host__ __device__ inline int cs_vregion(int L) { return kCsTile * cs_ldv(L) > 192 ? kCsTile * cs_ldv(L) : 192; }
static size_t cs_lds(int L, int D, int T) { return 4 * (static_cast<size_t>(T) * cs_lda(L, D) + cs_vregion(L)); }
static int cs_tile(int L, int D) { return cs_lds(L, D, kCsTile) <= kCsLdsCap ? kCsTile : kCsTile / 2; }
// a workgroup per tile up to what the GPU holds at once; beyond that the workgroups walk
static unsigned cs_fwd_grid(int64_t batch, int T) {
  const int64_t tiles = (batch + T - 1) / T;
  return static_cast<unsigned>(tiles < kCsFwdMaxGrid ? tiles : kCsFwdMaxGrid);
}
static unsigned cs_dx_grid(int64_t batch) {
  const int64_t need = (batch + 1) / 2;
  return static_cast<unsigned>(need < kCsDxMaxGrid ? need : kCsDxMaxGrid);
}
static int cs_elems(int L, int D, int nh) { return nh * D * (L * (L + 1) / 2); }
static int cs_total(int L, int D, int nh, int nv) { return cs_elems(L, D, nh) + nh * L + nv * L + nv; }
static int cs_runs(int64_t batch, int P) {
  const int chunks = (P + 255) / 256;
  int64_t r = (kCsDwTarget + chunks - 1) / chunks;
  if (r > kCsDwMaxRuns) r = kCsDwMaxRuns;
  const int64_t by_batch = (batch + kCsDwMinRun - 1) / kCsDwMinRun;
  if (r > by_batch) r = by_batch;
  return static_cast<int>(r < 1 ? 1 : r);
}

// acc[j] += X_j W^T for the nt <= kCsWin windows j: X_j[m][k] = xs[m lda + j D + k] (LDS; m < mlim, the other rows count as
// zeros and are not read), W[n][k] = w[n K + k] (global; n < nlim likewise), k < K, a multiple of 4.  One fetch of a weight
// feeds the MFMAs of all nt windows.  The bounds are AND masks on the loaded bits, as in mm16; nothing outside the operands is
// read: a window from nt on is skipped (nt is uniform over the wavefront).
__device__ __forceinline__ void cs_windows(const float* xs, const int lda, const int mlim, const float* w, const int K, const int nlim,
                                           const int D, const int nt, f32x4 (&acc)[kCsWin], const int col, const int quad) {
  const int mi = col < mlim ? col : mlim - 1, ni = col < nlim ? col : nlim - 1;
  int amask = col < mlim ? -1 : 0, bmask = col < nlim ? -1 : 0;
  asm volatile("" : "+v"(amask), "+v"(bmask));
  const float* ap = xs + mi * lda + quad;
  const float* bp = w + ni * K + quad;
  if (nt == kCsWin) {
    for (int k = 0; k < K; k += 4) {
      const float bv = __int_as_float(__float_as_int(bp[k]) & bmask);
#pragma unroll
      for (int j = 0; j < kCsWin; ++j) {
        const float av = __int_as_float(__float_as_int(ap[k + j * D]) & amask);
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[j], 0, 0, 0);
      }
    }
  } else {
    for (int k = 0; k < K; k += 4) {
      const float bv = __int_as_float(__float_as_int(bp[k]) & bmask);
#pragma unroll
      for (int j = 0; j < kCsWin; ++j) {
        if (j < nt) {
          const float av = __int_as_float(__float_as_int(ap[k + j * D]) & amask);
          acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[j], 0, 0, 0);
        }
      }
    }
  }
}

extern __shared__ __attribute__((aligned(16))) float cs_smem[];

__global__ __launch_bounds__(kCsFwdThreads) void caser_fwd_kernel(const CsFwd a) {
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6), col = lane & 15, quad = lane >> 4;
  const int nw = blockDim.x >> 6;
  const int L = a.L, D = a.D, nh = a.nh, nv = a.nv, T = a.T, lda = cs_lda(L, D), ldv = cs_ldv(L);
  const long long W = static_cast<long long>(nv) * D + static_cast<long long>(nh) * L;
  float* const X = cs_smem;                  // [T][L D + 4]
  float* const V = X + T * lda;              // w_v [16][pad4(L) + 4], zeros outside [n_v][L]
  const long long tiles = (a.B + T - 1) / T;
  const f32x4 zero = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int idx = tid; idx < cs_vregion(L); idx += blockDim.x) {
    const int v = idx / ldv, l = idx - v * ldv;
    V[idx] = (v < nv && l < L) ? a.wv[v * L + l] : 0.f;
  }

  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {                     // uniform over the workgroup
    const long long b0 = tile * T;
    const int nb = a.B - b0 < T ? static_cast<int>(a.B - b0) : T;
    __syncthreads();                         // the last tile's rows are read
    const int d4 = D >> 2, per = L * d4;
    for (int idx = tid; idx < T * per; idx += blockDim.x) {
      const int s = idx / per, rem = idx - s * per, l = rem / d4, q = rem - l * d4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (s < nb) v = *reinterpret_cast<const float4*>(a.x + (b0 + s) * a.sb + static_cast<long long>(l) * a.sl + 4 * q);
      *reinterpret_cast<float4*>(X + s * lda + l * D + 4 * q) = v;
    }
    __syncthreads();

    if (nh > 0) {
      for (int h = 1 + wv; h <= L; h += nw) {                                               // uniform over the wavefront
        const float* w = a.h.w[h - 1];
        const int K = h * D, nwin = L - h + 1;
        float best[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        int bt[4] = {0, 0, 0, 0};
        for (int t0 = 0; t0 < nwin; t0 += kCsWin) {
          const int nt = nwin - t0 < kCsWin ? nwin - t0 : kCsWin;
          f32x4 acc[kCsWin];
#pragma unroll
          for (int j = 0; j < kCsWin; ++j) acc[j] = zero;
          cs_windows(X + t0 * D, lda, T, w, K, nh, D, nt, acc, col, quad);
#pragma unroll
          for (int j = 0; j < kCsWin; ++j) {
            if (j < nt) {
#pragma unroll
              for (int r = 0; r < 4; ++r)
                if (acc[j][r] > best[r]) {   // strictly: the first maximal t wins, as in max_pool1d
                  best[r] = acc[j][r];
                  bt[r] = t0 + j;
                }
            }
          }
        }
        if (col < nh) {
          const float bias = a.h.b[h - 1][col];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int s = 4 * quad + r;
            if (s < nb) {
              const float v = best[r] + bias;
              const bool live = v > 0.f;
              const long long at = static_cast<long long>(h - 1) * nh + col;
              a.out[(b0 + s) * W + static_cast<long long>(nv) * D + at] = live ? v : 0.f;
              if (a.win != nullptr) a.win[(b0 + s) * (static_cast<long long>(L) * nh) + at] = static_cast<signed char>(live ? bt[r] : -1);
            }
          }
        }
      }
    }

    // The vertical rows, a wavefront per sample.  With klim = L < K = pad4(L) mm16 reads up to 3 rows of D floats behind the
    // sample's row: the next sample's row or, for the last one, the first 3 D - 4 floats of V, inside this workgroup's LDS.
    if (nv > 0) {
      for (int s = wv; s < nb; s += nw) {
        for (int n0 = 0; n0 < D; n0 += 16) {
          const f32x4 acc = mm16<false, false>(V, ldv, 0, nv, X + s * lda, D, n0, D, cs_pad4(L), L, zero, col, quad);
          const int d = n0 + col;
          if (d < D) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int v = 4 * quad + r;
              if (v < nv) a.out[(b0 + s) * W + v * D + d] = acc[r] + a.bv[v];
            }
          }
        }
      }
    }
  }
}

__global__ __launch_bounds__(256) void caser_dx_kernel(const CsBwd a) {
  float* const sg = cs_smem;                                  // [L n_h]: g where the winner is live, else 0
  int* const so = reinterpret_cast<int*>(cs_smem) + a.L * a.nh;   // [L n_h]: t* D, or -1
  const int tid = threadIdx.x, L = a.L, D = a.D, nh = a.nh, nv = a.nv, LD = L * D, LN = L * nh;
  const long long W = static_cast<long long>(nv) * D + LN;
  for (long long b = blockIdx.x; b < a.B; b += gridDim.x) {  // uniform over the workgroup
    const float* g = a.g + b * W;
    __syncthreads();                         // the last sample's winners are read
    for (int idx = tid; idx < LN; idx += blockDim.x) {
      const int t = a.win[b * LN + idx];
      sg[idx] = t >= 0 ? g[nv * D + idx] : 0.f;
      so[idx] = t >= 0 ? t * D : -1;
    }
    __syncthreads();
    for (int p = tid; p < LD; p += blockDim.x) {
      float acc = 0.f;
      for (int h = 1; h <= L; ++h) {
        const float* w = a.h.w[h - 1];
        const int K = h * D;
        for (int f = 0; f < nh; ++f) {
          const int off = so[(h - 1) * nh + f], o = p - off;
          if (off >= 0 && o >= 0 && o < K) acc += sg[(h - 1) * nh + f] * w[f * K + o];
        }
      }
      const int l = p / D, d = p - l * D;
      for (int v = 0; v < nv; ++v) acc += a.wv[v * L + l] * g[v * D + d];
      a.dx[b * LD + p] = acc;
    }
  }
}

__global__ __launch_bounds__(256) void caser_dw_kernel(const CsBwd a) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= a.P) return;
  const int L = a.L, D = a.D, nh = a.nh, nv = a.nv, LN = L * nh;
  const long long W = static_cast<long long>(nv) * D + LN;
  const long long lo = blockIdx.y * a.run, hi = lo + a.run < a.B ? lo + a.run : a.B;
  float acc = 0.f;
  if (e < a.E) {                             // dW_h[h - 1][f, i, d]: row = n_h h (h - 1) / 2 + f h + i of D floats
    const int row = e / D, d = e - row * D;
    int h = 1;
    while (h < L && nh * (h * (h + 1) / 2) <= row) ++h;
    const int rem = row - nh * (h * (h - 1) / 2), f = rem / h, i = rem - f * h;
    const long long at = static_cast<long long>(h - 1) * nh + f;
    for (long long b = lo; b < hi; ++b) {
      const int t = a.win[b * LN + at];
      if (t >= 0) acc += a.g[b * W + nv * D + at] * a.x[b * a.sb + static_cast<long long>(t + i) * a.sl + d];
    }
  } else if (e < a.E + LN) {                 // db_h[h - 1][f]
    const int at = e - a.E;
    for (long long b = lo; b < hi; ++b)
      if (a.win[b * LN + at] >= 0) acc += a.g[b * W + nv * D + at];
  } else if (e < a.E + LN + nv * L) {        // dW_v[v, l]
    const int at = e - a.E - LN, v = at / L, l = at - v * L;
    for (long long b = lo; b < hi; ++b) {
      const float* gr = a.g + b * W + v * D;
      const float* xr = a.x + b * a.sb + static_cast<long long>(l) * a.sl;
      for (int d = 0; d < D; ++d) acc += gr[d] * xr[d];
    }
  } else {                                   // db_v[v]
    const int v = e - a.E - LN - nv * L;
    for (long long b = lo; b < hi; ++b) {
      const float* gr = a.g + b * W + v * D;
      for (int d = 0; d < D; ++d) acc += gr[d];
    }
  }
  a.part[static_cast<long long>(blockIdx.y) * a.P + e] = acc;
}

__global__ __launch_bounds__(256) void caser_tail_kernel(const CsTail t) {
  __shared__ float sm[16][17];
  const int c = threadIdx.x & 15, r = threadIdx.x >> 4, e = blockIdx.x * 16 + c;
  colsum16(t.part, t.R, t.P, e, r, c, sm);
  if (r != 0 || e >= t.P) return;
  const float s = sm[0][c];
  const int LN = t.L * t.nh;
  if (e < t.E) {
    const int row = e / t.D;
    int h = 1;
    while (h < t.L && t.nh * (h * (h + 1) / 2) <= row) ++h;
    float* dst = t.h.dw[h - 1];
    if (dst != nullptr) dst[e - t.nh * (h * (h - 1) / 2) * t.D] = s;
  } else if (e < t.E + LN) {
    const int at = e - t.E, h1 = at / t.nh;
    float* dst = t.h.db[h1];
    if (dst != nullptr) dst[at - h1 * t.nh] = s;
  } else if (e < t.E + LN + t.nv * t.L) {
    if (t.dwv != nullptr) t.dwv[e - t.E - LN] = s;
  } else if (t.dbv != nullptr) {
    t.dbv[e - t.E - LN - t.nv * t.L] = s;
  }
}

static int cs_check(const char* what, int64_t batch, int32_t L, int32_t D, int32_t nh, int32_t nv, int32_t dtype) {
  if (batch < 0) return fail(RBX_ERR_INVALID, "%s: batch=%lld", what, static_cast<long long>(batch));
  if (!rbx_caser_supported(L, D, nh, nv))
    return fail(RBX_ERR_UNSUPPORTED, "%s: L=%d in [1,%d], D=%d a multiple of 4 in [4,%d], n_h=%d in [0,%d], n_v=%d in [0,%d], n_h + n_v > 0",
                what, L, kCsMaxL, D, kCsMaxD, nh, kCsMaxNh, nv, kCsMaxNv);
  if (dtype != RBX_F32) return fail(RBX_ERR_UNSUPPORTED, "%s: tensor dtype code %d (float32 only)", what, dtype);
  return RBX_OK;
}

static int cs_ptrs(const char* what, const void* const* w_h, const void* const* b_h, int L, int nh, bool need_b, CsPtrs* out) {
  *out = CsPtrs{};
  if (nh == 0) return RBX_OK;
  if (w_h == nullptr || (need_b && b_h == nullptr)) return fail(RBX_ERR_INVALID, "%s: NULL pointer array", what);
  for (int h = 0; h < L; ++h) {
    if (w_h[h] == nullptr || (need_b && b_h[h] == nullptr)) return fail(RBX_ERR_INVALID, "%s: NULL filter tensor %d", what, h);
    out->w[h] = static_cast<const float*>(w_h[h]);
    out->b[h] = need_b ? static_cast<const float*>(b_h[h]) : nullptr;
  }
  return RBX_OK;
}

}  // namespace rbx

extern "C" int rbx_caser_supported(int32_t L, int32_t D, int32_t n_h, int32_t n_v) {
  using namespace rbx;
  return L >= 1 && L <= kCsMaxL && D >= 4 && D <= kCsMaxD && (D & 3) == 0 && n_h >= 0 && n_h <= kCsMaxNh && n_v >= 0 &&
         n_v <= kCsMaxNv && n_h + n_v > 0;
}

extern "C" int rbx_caser_fwd(const float* d_x, int64_t x_stride_b, int64_t x_stride_l, const float* d_w_v, const float* d_b_v,
                             const void* const* w_h, const void* const* b_h, int64_t batch, int32_t L, int32_t D, int32_t n_h,
                             int32_t n_v, int32_t dtype, float* d_out, int8_t* d_win, void* stream) {
  using namespace rbx;
  int rc = cs_check("caser_fwd", batch, L, D, n_h, n_v, dtype);
  if (rc != RBX_OK) return rc;
  if (batch == 0) return RBX_OK;
  if (!d_x || !d_out || (n_v > 0 && (!d_w_v || !d_b_v))) return fail(RBX_ERR_INVALID, "caser_fwd: NULL tensor");
  if (!aligned16(d_x) || (x_stride_b & 3) || (x_stride_l & 3) || x_stride_l < D || x_stride_b < 0 || x_stride_l > INT_MAX)
    return fail(RBX_ERR_UNSUPPORTED, "caser_fwd: x must be 16-byte aligned with strides that are multiples of 4 floats");
  CsFwd a = {};
  rc = cs_ptrs("caser_fwd", w_h, b_h, L, n_h, true, &a.h);
  if (rc != RBX_OK) return rc;
  a.x = d_x; a.wv = d_w_v; a.bv = d_b_v; a.out = d_out; a.win = reinterpret_cast<signed char*>(d_win);
  a.B = batch; a.sb = x_stride_b; a.sl = static_cast<int>(x_stride_l);
  a.L = L; a.D = D; a.nh = n_h; a.nv = n_v; a.T = cs_tile(L, D);
  const size_t lds = cs_lds(L, D, a.T);
  rc = allow_lds("caser_fwd", caser_fwd_kernel, lds);
  if (rc != RBX_OK) return rc;
  hipLaunchKernelGGL(caser_fwd_kernel, dim3(cs_fwd_grid(batch, a.T)), dim3(kCsFwdThreads), lds, as_stream(stream), a);
  return check_launch("caser_fwd");
}

extern "C" size_t rbx_caser_bwd_workspace_size(int64_t batch, int32_t L, int32_t D, int32_t n_h, int32_t n_v) {
  using namespace rbx;
  if (batch <= 0 || !rbx_caser_supported(L, D, n_h, n_v)) return 0;
  const int P = cs_total(L, D, n_h, n_v);
  return static_cast<size_t>(cs_runs(batch, P)) * P * sizeof(float);
}

extern "C" int rbx_caser_bwd(const float* d_dout, const float* d_x, int64_t x_stride_b, int64_t x_stride_l, const float* d_w_v,
                             const void* const* w_h, const int8_t* d_win, int64_t batch, int32_t L, int32_t D, int32_t n_h,
                             int32_t n_v, int32_t dtype, float* d_dx, float* d_dw_v, float* d_db_v, void* const* dw_h,
                             void* const* db_h, void* d_workspace, size_t workspace_bytes, void* stream) {
  using namespace rbx;
  int rc = cs_check("caser_bwd", batch, L, D, n_h, n_v, dtype);
  if (rc != RBX_OK) return rc;
  if (batch == 0) return RBX_OK;
  if (!d_dout || !d_x || (n_v > 0 && !d_w_v) || (n_h > 0 && !d_win)) return fail(RBX_ERR_INVALID, "caser_bwd: NULL tensor");
  if (x_stride_b < 0 || x_stride_l < D || x_stride_l > INT_MAX) return fail(RBX_ERR_UNSUPPORTED, "caser_bwd: strides of x");
  const bool want_w = d_dw_v || d_db_v || dw_h || db_h;
  if (want_w && (d_workspace == nullptr || workspace_bytes < rbx_caser_bwd_workspace_size(batch, L, D, n_h, n_v)))
    return fail(RBX_ERR_WORKSPACE, "caser_bwd: workspace too small");
  if (!want_w && !d_dx) return RBX_OK;
  CsBwd a = {};
  rc = cs_ptrs("caser_bwd", w_h, nullptr, L, n_h, false, &a.h);
  if (rc != RBX_OK) return rc;
  a.x = d_x; a.g = d_dout; a.win = reinterpret_cast<const signed char*>(d_win); a.wv = d_w_v; a.dx = d_dx;
  a.part = static_cast<float*>(d_workspace);
  a.B = batch; a.sb = x_stride_b; a.sl = static_cast<int>(x_stride_l);
  a.L = L; a.D = D; a.nh = n_h; a.nv = n_v; a.E = cs_elems(L, D, n_h); a.P = cs_total(L, D, n_h, n_v);
  hipStream_t s = as_stream(stream);
  if (d_dx) {
    const size_t lds = static_cast<size_t>(8) * (L * n_h > 0 ? L * n_h : 1);
    rc = allow_lds("caser_dx", caser_dx_kernel, lds);
    if (rc != RBX_OK) return rc;
    hipLaunchKernelGGL(caser_dx_kernel, dim3(cs_dx_grid(batch)), dim3(256), lds, s, a);
  }
  if (want_w) {
    const int R = cs_runs(batch, a.P);
    a.run = (batch + R - 1) / R;
    hipLaunchKernelGGL(caser_dw_kernel, dim3((a.P + 255) / 256, R), dim3(256), 0, s, a);
    CsTail t = {};
    t.part = a.part; t.dwv = d_dw_v; t.dbv = d_db_v;
    t.R = R; t.P = a.P; t.E = a.E; t.L = L; t.D = D; t.nh = n_h; t.nv = n_v;
    for (int h = 0; h < L && n_h > 0; ++h) {
      t.h.dw[h] = dw_h ? static_cast<float*>(dw_h[h]) : nullptr;
      t.h.db[h] = db_h ? static_cast<float*>(db_h[h]) : nullptr;
    }
    hipLaunchKernelGGL(caser_tail_kernel, dim3((a.P + 15) / 16), dim3(256), 0, s, t);
  }
  return check_launch("caser_bwd");
}
