// rbx_crossmix.hip -- DCN-V2's mixture of low-rank cross experts (gfx950, wave64), one layer per call.  Replaces, under
// third_party/rechub/basic/layers.py (CrossNetMix) and models/ranking/dcn_v2.py, four matmuls and a Hadamard product per expert,
// a torch.stack into [B, n, E] and a matmul with the softmax per layer.  x0, x_l [B, n]; V, U [E, n, r]; C [E, r, r]; G [E, n]
// (the E bias-free Linear(n, 1) gates, shared by all layers); b [n]:
//
//   z_e = x_l . G_e      p = softmax_e(z)      h1_e = tanh(x_l V_e)      h2_e = tanh(h1_e C_e^T)
//   mix = sum_e p_e (h2_e U_e^T) + b           out = x_l + x0 * mix      (sum_e p_e = 1: the reference's per-expert mixture)
//
// cm_fwd_kernel  a workgroup stages 16 rows of x_l in LDS once.  [V_1 .. V_E | G^T] is applied on v_mfma_f32_16x16x4_f32 (exact
//                fp32; rows = samples, k = input column), a wavefront per block of 16 output columns, the weights read through
//                L2; tanh, the E products with C, tanh, the softmax and the p_e scaling stay in LDS; the projection back through
//                U runs on the MFMA and its epilogue writes x_l + x0 (mix + b) with a row stride.  Nothing of size [B, E r] or
//                [B, n, E] is written.
// cm_bwd_kernel  the row side of the backward for the same tile: recomputes h1, h2, p and mix from x_l (the forward saves no
//                activation), writes dx_l = dout + sum_e da1_e V_e^T + dz G and dx0 (+)= dout * mix, and leaves the operands of
//                the weight gradients in the workspace: p_e h2_e, da1, da2, h1 [B, E r] and dz [B, E].
// cm_xty_kernel  out[i, j] = sum_b A[b, i] (A2[b, i]) B[b, j] over a chunk of rows on the MFMA (k = 4 rows), one 16 x 64 block per
//                wavefront, into per-chunk partials; cm_tail_kernel adds the chunks in ascending order.  dU (A = dout * x0),
//                dV, dC (one z-slice per expert), dG and db come from it.
// No atomics, every sum in a fixed order: two runs give the same bits.  No call allocates or synchronises.
#include <math.h>

#include "rbx_internal.h"

namespace rbx {

constexpr int kCmTile = 16;                  // rows per workgroup = rows of the MFMA
constexpr int kCmBlock = 256;
constexpr int kCmMaxN = 640, kCmMaxE = 8, kCmMaxER = 256;
constexpr int kCmChunks = 16;                // row chunks of the weight-gradient partials
constexpr size_t kCmLdsCap = 160 * 1024;

__host__ __device__ inline int cm_xs(int n) { return ((n + 3) & ~3) + 4; }     // row stride of an [16, n] tile, zero padded
__host__ __device__ inline int cm_hs(int er) { return er + 4; }                // row stride of an [16, E r] tile

static bool cm_rank_ok(int r) { return r == 4 || r == 8 || r == 16 || r == 32 || r == 64; }

struct CmArgs {
  const float *x0, *xl;      // x[b stride + k]
  long long x0s, xls;
  const float *U, *V, *C, *G, *b;
  float* out;                // forward
  long long os;
  const float* dout;         // backward
  long long ds;
  float *dxl, *dx0;
  long long dxls, dx0s;
  float *ph2, *da1, *da2, *h1, *dz;      // [B, E r] x 4, [B, E]
  long long B;
  int n, E, r, rsh, acc;     // rsh = log2 r; acc: dx0 is added to
};

// acc[16, 16 cb ..] = A[16, K = n] . W, W's column c = (expert c / r, rank c % r) of a [E, n, r] stack, then (G != NULL) the E gate
// columns G[e, :].  A sits in LDS with stride S, zero padded to a multiple of 4.  A wavefront takes column blocks wave, wave + 4, ..
template <typename Epi>
__device__ __forceinline__ void cm_gemm_in(const float* As, int S, const float* W, const float* G, int n, int E, int r, int rsh,
                                           Epi epi) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, quad = lane >> 4;
  const int ER = E * r, cols = ER + (G != nullptr ? E : 0), ksteps = (n + 3) >> 2;
  for (int cb = wave; cb * 16 < cols; cb += 4) {
    const int c = 16 * cb + col;
    const float* base = nullptr;
    int kst = 0;
    if (c < ER) {
      base = W + (c >> rsh) * n * r + (c & (r - 1));
      kst = r;
    } else if (c < cols) {
      base = G + (c - ER) * n;
      kst = 1;
    }
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < ksteps; ++s) {
      const int k = 4 * s + quad;
      const float bv = (base != nullptr && k < n) ? base[k * kst] : 0.f;
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(As[col * S + k], bv, acc, 0, 0, 0);
    }
    if (c < cols) {
#pragma unroll
      for (int t = 0; t < 4; ++t) epi(4 * quad + t, c, acc[t]);
    }
  }
}

// acc[16, 16 cb ..] = A[16, K = E r] . W^T, element (k = c, m) = W[expert c / r, m, rank c % r]: the projection back to n columns
template <typename Epi>
__device__ __forceinline__ void cm_gemm_out(const float* As, int HS, const float* W, int n, int E, int r, int rsh, Epi epi) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, quad = lane >> 4;
  const int ksteps = (E * r) >> 2;
  for (int cb = wave; cb * 16 < n; cb += 4) {
    const int m = 16 * cb + col;
    const float* base = W + (m < n ? m : 0) * r;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < ksteps; ++s) {
      const int c = 4 * s + quad;
      const float bv = m < n ? base[(c >> rsh) * n * r + (c & (r - 1))] : 0.f;
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(As[col * HS + c], bv, acc, 0, 0, 0);
    }
    if (m < n) {
#pragma unroll
      for (int t = 0; t < 4; ++t) epi(4 * quad + t, m, acc[t]);
    }
  }
}

// h1s = tanh(x V), h2s = tanh(h1 C^T), ps = softmax(x G^T) of the staged tile xs; ends with a barrier
__device__ __forceinline__ void cm_forward_tile(const CmArgs& a, const float* xs, float* h1s, float* h2s, float* ps) {
  const int n = a.n, E = a.E, r = a.r, rsh = a.rsh, ER = E * r, S = cm_xs(n), HS = cm_hs(ER);
  cm_gemm_in(xs, S, a.V, a.G, n, E, r, rsh, [&](int row, int c, float v) {
    if (c < ER) h1s[row * HS + c] = tanhf(v);
    else ps[row * kCmMaxE + (c - ER)] = v;
  });
  __syncthreads();
  for (int idx = threadIdx.x; idx < kCmTile * ER; idx += kCmBlock) {
    const int row = idx / ER, c = idx - row * ER, e = c >> rsh, i = c & (r - 1);
    const float* cr = a.C + (e * r + i) * r;
    const float* hr = h1s + row * HS + e * r;
    float acc = 0.f;
    for (int j = 0; j < r; ++j) acc = fma_rn(cr[j], hr[j], acc);
    h2s[row * HS + c] = tanhf(acc);
  }
  if (threadIdx.x < kCmTile) {
    float* z = ps + threadIdx.x * kCmMaxE;
    float mx = z[0];
    for (int e = 1; e < E; ++e) mx = fmaxf(mx, z[e]);
    float sum = 0.f;
    for (int e = 0; e < E; ++e) {
      const float w = expf(z[e] - mx);
      z[e] = w;
      sum += w;
    }
    const float inv = 1.f / sum;
    for (int e = 0; e < E; ++e) z[e] *= inv;
  }
  __syncthreads();
}

__device__ __forceinline__ void cm_stage_x(const CmArgs& a, long long b0, float* xs) {
  const int S = cm_xs(a.n);
  for (int idx = threadIdx.x; idx < kCmTile * S; idx += kCmBlock) {
    const int row = idx / S, k = idx - row * S;
    xs[idx] = (b0 + row < a.B && k < a.n) ? a.xl[(b0 + row) * a.xls + k] : 0.f;
  }
}

__global__ __launch_bounds__(kCmBlock) void cm_fwd_kernel(const CmArgs a) {
  extern __shared__ __attribute__((aligned(16))) float cm_lds[];
  const int n = a.n, E = a.E, r = a.r, rsh = a.rsh, ER = E * r, S = cm_xs(n), HS = cm_hs(ER);
  float* xs = cm_lds;                        // [16][S]
  float* h1s = xs + kCmTile * S;             // [16][HS]
  float* h2s = h1s + kCmTile * HS;           // [16][HS]
  float* ps = h2s + kCmTile * HS;            // [16][8]
  const long long b0 = static_cast<long long>(blockIdx.x) * kCmTile;
  cm_stage_x(a, b0, xs);
  __syncthreads();
  cm_forward_tile(a, xs, h1s, h2s, ps);
  for (int idx = threadIdx.x; idx < kCmTile * ER; idx += kCmBlock) {
    const int row = idx / ER, c = idx - row * ER;
    h2s[row * HS + c] = mul_rn(ps[row * kCmMaxE + (c >> rsh)], h2s[row * HS + c]);
  }
  __syncthreads();
  cm_gemm_out(h2s, HS, a.U, n, E, r, rsh, [&](int row, int m, float v) {
    const long long b = b0 + row;
    if (b < a.B) a.out[b * a.os + m] = fma_rn(a.x0[b * a.x0s + m], add_rn(v, a.b[m]), xs[row * S + m]);
  });
}

__global__ __launch_bounds__(kCmBlock) void cm_bwd_kernel(const CmArgs a) {
  extern __shared__ __attribute__((aligned(16))) float cm_lds[];
  const int n = a.n, E = a.E, r = a.r, rsh = a.rsh, ER = E * r, S = cm_xs(n), HS = cm_hs(ER);
  float* xs = cm_lds;                        // [16][S]   x_l
  float* dms = xs + kCmTile * S;             // [16][S]   dmix = dout * x0
  float* h1s = dms + kCmTile * S;            // [16][HS]
  float* h2s = h1s + kCmTile * HS;           // [16][HS]
  float* t1s = h2s + kCmTile * HS;           // [16][HS]  p h2, then da1
  float* t2s = t1s + kCmTile * HS;           // [16][HS]  dg, then da2
  float* ps = t2s + kCmTile * HS;            // [16][8]
  float* dps = ps + kCmTile * kCmMaxE;       // [16][8]   dp, then dz
  const long long b0 = static_cast<long long>(blockIdx.x) * kCmTile;
  cm_stage_x(a, b0, xs);
  for (int idx = threadIdx.x; idx < kCmTile * S; idx += kCmBlock) {
    const int row = idx / S, k = idx - row * S;
    const long long b = b0 + row;
    dms[idx] = (b < a.B && k < n) ? mul_rn(a.dout[b * a.ds + k], a.x0[b * a.x0s + k]) : 0.f;
  }
  __syncthreads();
  cm_forward_tile(a, xs, h1s, h2s, ps);
  for (int idx = threadIdx.x; idx < kCmTile * ER; idx += kCmBlock) {
    const int row = idx / ER, c = idx - row * ER;
    const long long b = b0 + row;
    const float v = mul_rn(ps[row * kCmMaxE + (c >> rsh)], h2s[row * HS + c]);
    t1s[row * HS + c] = v;
    if (b < a.B) {
      a.ph2[b * ER + c] = v;
      a.h1[b * ER + c] = h1s[row * HS + c];
    }
  }
  __syncthreads();
  // dx0 (+)= dout * (mix + b), mix recomputed; dg = dmix U
  cm_gemm_out(t1s, HS, a.U, n, E, r, rsh, [&](int row, int m, float v) {
    const long long b = b0 + row;
    if (b < a.B) {
      float* p = a.dx0 + b * a.dx0s + m;
      const float g = mul_rn(a.dout[b * a.ds + m], add_rn(v, a.b[m]));
      *p = a.acc ? add_rn(*p, g) : g;
    }
  });
  cm_gemm_in(dms, S, a.U, nullptr, n, E, r, rsh, [&](int row, int c, float v) { t2s[row * HS + c] = v; });
  __syncthreads();
  if (threadIdx.x < kCmTile * E) {
    const int row = threadIdx.x / E, e = threadIdx.x - row * E;
    const float* g = t2s + row * HS + e * r;
    const float* h = h2s + row * HS + e * r;
    float acc = 0.f;
    for (int j = 0; j < r; ++j) acc = fma_rn(g[j], h[j], acc);
    dps[row * kCmMaxE + e] = acc;
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < kCmTile * ER; idx += kCmBlock) {          // da2 = p dg (1 - h2^2)
    const int row = idx / ER, c = idx - row * ER;
    const float h = h2s[row * HS + c];
    const float v = mul_rn(mul_rn(ps[row * kCmMaxE + (c >> rsh)], t2s[row * HS + c]), fma_rn(-h, h, 1.f));
    t2s[row * HS + c] = v;
    if (b0 + row < a.B) a.da2[(b0 + row) * ER + c] = v;
  }
  __syncthreads();
  if (threadIdx.x < kCmTile) {                                                 // dz = p (dp - sum_e p_e dp_e)
    const int row = threadIdx.x;
    float s = 0.f;
    for (int e = 0; e < E; ++e) s = fma_rn(ps[row * kCmMaxE + e], dps[row * kCmMaxE + e], s);
    for (int e = 0; e < E; ++e) {
      const float v = mul_rn(ps[row * kCmMaxE + e], dps[row * kCmMaxE + e] - s);
      dps[row * kCmMaxE + e] = v;
      if (b0 + row < a.B) a.dz[(b0 + row) * E + e] = v;
    }
  }
  for (int idx = threadIdx.x; idx < kCmTile * ER; idx += kCmBlock) {          // da1 = (da2 C)(1 - h1^2)
    const int row = idx / ER, c = idx - row * ER, e = c >> rsh, j = c & (r - 1);
    const float* cc = a.C + e * r * r + j;
    const float* g = t2s + row * HS + e * r;
    float acc = 0.f;
    for (int i = 0; i < r; ++i) acc = fma_rn(g[i], cc[i * r], acc);
    const float h = h1s[row * HS + c];
    const float v = mul_rn(acc, fma_rn(-h, h, 1.f));
    t1s[row * HS + c] = v;
    if (b0 + row < a.B) a.da1[(b0 + row) * ER + c] = v;
  }
  __syncthreads();
  cm_gemm_out(t1s, HS, a.V, n, E, r, rsh, [&](int row, int m, float v) {
    const long long b = b0 + row;
    if (b < a.B) {
      float g = 0.f;
      for (int e = 0; e < E; ++e) g = fma_rn(dps[row * kCmMaxE + e], a.G[e * n + m], g);
      a.dxl[b * a.dxls + m] = add_rn(a.dout[b * a.ds + m], add_rn(v, g));
    }
  });
}

// ---- the weight gradients: sums over the batch ------------------------------------------------------------------------------
struct XtyArgs {
  const float* A;            // A[b lda + z az + i], i < I
  const float* A2;           // optional factor of A, A2[b lda2 + i]
  const float* Bm;           // Bm[b ldb + z bz + j], j < J; NULL: ones
  long long lda, lda2, ldb;
  int az, bz;
  float* part;               // [chunks][Z][I][J]
  long long B, rpc;          // rows per chunk, a multiple of 4
  int I, J;
};

__global__ __launch_bounds__(kCmBlock) void cm_xty_kernel(const XtyArgs x) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, quad = lane >> 4;
  const int tj4 = (x.J + 63) / 64, wt = blockIdx.y * 4 + wave, ti = wt / tj4, tj = wt - ti * tj4;
  if (ti * 16 >= x.I) return;
  const int z = blockIdx.z, i = 16 * ti + col, jb = 64 * tj + col;
  const long long c0 = x.rpc * blockIdx.x, c1 = c0 + x.rpc < x.B ? c0 + x.rpc : x.B;
  const float* A = x.A + z * x.az;
  const float* Bm = x.Bm != nullptr ? x.Bm + z * x.bz : nullptr;
  f32x4 acc[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (long long b = c0; b < c1; b += 4) {
    const long long row = b + quad;
    const bool ok = row < c1;
    float av = 0.f;
    if (ok && i < x.I) {
      av = A[row * x.lda + i];
      if (x.A2 != nullptr) av = mul_rn(av, x.A2[row * x.lda2 + i]);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = jb + 16 * q;
      float bv = 0.f;
      if (ok && j < x.J) bv = Bm != nullptr ? Bm[row * x.ldb + j] : 1.f;
      acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[q], 0, 0, 0);
    }
  }
  float* o = x.part + (static_cast<long long>(blockIdx.x) * gridDim.z + z) * x.I * x.J;
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int ii = 16 * ti + 4 * quad + t, j = jb + 16 * q;
      if (ii < x.I && j < x.J) o[static_cast<long long>(ii) * x.J + j] = acc[q][t];
    }
}

// out (+)= the chunks of part [chunks][Z I J], ascending.  split_r > 0: element (i, j) of a [I, J = E r] result lands at
// [e = j / r][i][j % r] -- the [E, n, r] layout of U and V.
__global__ __launch_bounds__(256) void cm_tail_kernel(const float* part, int chunks, long long total, int I, int J, int split_r,
                                                      int accumulate, float* out) {
  const long long idx = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
  if (idx >= total) return;
  float s = 0.f;
  for (int k = 0; k < chunks; ++k) s += part[k * total + idx];
  long long o = idx;
  if (split_r > 0) {
    const int i = static_cast<int>(idx / J), j = static_cast<int>(idx - static_cast<long long>(i) * J);
    o = (static_cast<long long>(j / split_r) * I + i) * split_r + (j % split_r);
  }
  out[o] = accumulate ? out[o] + s : s;
}

static size_t cm_fwd_lds(int n, int er) { return sizeof(float) * (kCmTile * (cm_xs(n) + 2 * cm_hs(er)) + kCmTile * kCmMaxE); }
static size_t cm_bwd_lds(int n, int er) { return sizeof(float) * (kCmTile * (2 * cm_xs(n) + 4 * cm_hs(er)) + 2 * kCmTile * kCmMaxE); }

static void cm_split(long long B, int* chunks, long long* rpc) {
  long long per = (B + kCmChunks - 1) / kCmChunks;
  per = (per + 63) / 64 * 64;
  *rpc = per;
  *chunks = static_cast<int>((B + per - 1) / per);
}

static size_t cm_part_floats(int n, int E, int r) {
  const size_t er = static_cast<size_t>(E) * r;
  size_t m = static_cast<size_t>(n) * er;
  if (er * r > m) m = er * r;
  if (static_cast<size_t>(E) * n > m) m = static_cast<size_t>(E) * n;
  return m * kCmChunks;
}

static int cm_log2(int r) {
  int s = 0;
  while ((1 << s) < r) ++s;
  return s;
}

static int cm_check(const char* what, int64_t batch, int n, int E, int r, int dtype, int64_t x0s, int64_t xls) {
  if (batch < 0) return fail(RBX_ERR_INVALID, "%s: batch=%lld", what, static_cast<long long>(batch));
  if (!rbx_crossmix_supported(n, E, r, dtype))
    return fail(RBX_ERR_UNSUPPORTED, "%s: needs float32, n=%d in [1,%d], experts=%d in [1,%d], rank=%d in {4,8,16,32,64}, experts*rank <= %d",
                what, n, kCmMaxN, E, kCmMaxE, r, kCmMaxER);
  if (batch == 0) return RBX_OK;
  if (x0s < n || xls < n) return fail(RBX_ERR_INVALID, "%s: a row stride is shorter than n=%d", what, n);
  if ((batch + kCmTile - 1) / kCmTile > INT_MAX) return fail(RBX_ERR_UNSUPPORTED, "%s: batch=%lld is too large", what, static_cast<long long>(batch));
  return RBX_OK;
}

static int cm_xty(hipStream_t s, const XtyArgs& x, int Z, int chunks, int split_r, int accumulate, float* out) {
  const int tiles = ((x.I + 15) / 16) * ((x.J + 63) / 64);
  hipLaunchKernelGGL(cm_xty_kernel, dim3(chunks, (tiles + 3) / 4, Z), dim3(kCmBlock), 0, s, x);
  const long long total = static_cast<long long>(Z) * x.I * x.J;
  hipLaunchKernelGGL(cm_tail_kernel, dim3(static_cast<unsigned>((total + 255) / 256)), dim3(256), 0, s, x.part, chunks, total, x.I, x.J,
                     split_r, accumulate, out);
  return check_launch("crossmix weight gradients");
}

}  // namespace rbx

extern "C" int rbx_crossmix_supported(int32_t n, int32_t experts, int32_t rank, int32_t dtype) {
  using namespace rbx;
  if (dtype != RBX_F32 || n < 1 || n > kCmMaxN || experts < 1 || experts > kCmMaxE || !cm_rank_ok(rank)) return 0;
  if (experts * rank > kCmMaxER) return 0;
  return cm_bwd_lds(n, experts * rank) <= kCmLdsCap;
}

extern "C" int rbx_crossmix_fwd(const float* d_x0, int64_t x0_stride, const float* d_xl, int64_t xl_stride, const float* d_u,
                                const float* d_v, const float* d_c, const float* d_g, const float* d_b, int64_t batch, int32_t n,
                                int32_t experts, int32_t rank, int32_t dtype, float* d_out, int64_t out_stride, void* stream) {
  using namespace rbx;
  const int rc = cm_check("crossmix_fwd", batch, n, experts, rank, dtype, x0_stride, xl_stride);
  if (rc != RBX_OK || batch == 0) return rc;
  if (!d_x0 || !d_xl || !d_u || !d_v || !d_c || !d_g || !d_b || !d_out) return fail(RBX_ERR_INVALID, "crossmix_fwd: NULL pointer");
  if (out_stride < n) return fail(RBX_ERR_INVALID, "crossmix_fwd: out_stride=%lld is shorter than a row", static_cast<long long>(out_stride));
  CmArgs a{};
  a.x0 = d_x0; a.x0s = x0_stride; a.xl = d_xl; a.xls = xl_stride; a.U = d_u; a.V = d_v; a.C = d_c; a.G = d_g; a.b = d_b;
  a.out = d_out; a.os = out_stride; a.B = batch; a.n = n; a.E = experts; a.r = rank; a.rsh = cm_log2(rank);
  const size_t lds = cm_fwd_lds(n, experts * rank);
  const int rc_lds = allow_lds("crossmix_fwd", cm_fwd_kernel, lds);
  if (rc_lds != RBX_OK) return rc_lds;
  hipLaunchKernelGGL(cm_fwd_kernel, dim3(static_cast<unsigned>((batch + kCmTile - 1) / kCmTile)), dim3(kCmBlock), lds,
                     as_stream(stream), a);
  return check_launch("crossmix_fwd");
}

extern "C" size_t rbx_crossmix_bwd_workspace_size(int64_t batch, int32_t n, int32_t experts, int32_t rank) {
  using namespace rbx;
  if (batch <= 0 || !rbx_crossmix_supported(n, experts, rank, RBX_F32)) return 0;
  const size_t rows = static_cast<size_t>(batch), er = static_cast<size_t>(experts) * rank;
  return sizeof(float) * (rows * (4 * er + experts) + cm_part_floats(n, experts, rank));
}

extern "C" int rbx_crossmix_bwd(const float* d_dout, int64_t dout_stride, const float* d_x0, int64_t x0_stride, const float* d_xl,
                                int64_t xl_stride, const float* d_u, const float* d_v, const float* d_c, const float* d_g,
                                const float* d_b, int64_t batch, int32_t n, int32_t experts, int32_t rank, int32_t dtype,
                                int32_t accumulate, float* d_dxl, int64_t dxl_stride, float* d_dx0, int64_t dx0_stride, float* d_du,
                                float* d_dv, float* d_dc, float* d_dg, float* d_db, void* d_workspace, size_t workspace_bytes,
                                void* stream) {
  using namespace rbx;
  const int rc = cm_check("crossmix_bwd", batch, n, experts, rank, dtype, x0_stride, xl_stride);
  if (rc != RBX_OK || batch == 0) return rc;
  if (!d_dout || !d_x0 || !d_xl || !d_u || !d_v || !d_c || !d_g || !d_b || !d_dxl || !d_dx0 || !d_du || !d_dv || !d_dc || !d_dg ||
      !d_db || !d_workspace)
    return fail(RBX_ERR_INVALID, "crossmix_bwd: NULL pointer");
  if (dout_stride < n || dxl_stride < n || dx0_stride < n)
    return fail(RBX_ERR_INVALID, "crossmix_bwd: a row stride is shorter than n=%d", n);
  if (workspace_bytes < rbx_crossmix_bwd_workspace_size(batch, n, experts, rank))
    return fail(RBX_ERR_WORKSPACE, "crossmix_bwd: workspace of %zu bytes is too small", workspace_bytes);
  const int E = experts, r = rank, ER = E * r;
  const size_t rows = static_cast<size_t>(batch);
  float* ws = static_cast<float*>(d_workspace);
  CmArgs a{};
  a.x0 = d_x0; a.x0s = x0_stride; a.xl = d_xl; a.xls = xl_stride; a.U = d_u; a.V = d_v; a.C = d_c; a.G = d_g; a.b = d_b;
  a.dout = d_dout; a.ds = dout_stride; a.dxl = d_dxl; a.dxls = dxl_stride; a.dx0 = d_dx0; a.dx0s = dx0_stride;
  a.ph2 = ws; a.da1 = a.ph2 + rows * ER; a.da2 = a.da1 + rows * ER; a.h1 = a.da2 + rows * ER; a.dz = a.h1 + rows * ER;
  float* part = a.dz + rows * E;
  a.B = batch; a.n = n; a.E = E; a.r = r; a.rsh = cm_log2(r); a.acc = accumulate != 0;
  hipStream_t s = as_stream(stream);
  const size_t lds = cm_bwd_lds(n, ER);
  const int rc_lds = allow_lds("crossmix_bwd", cm_bwd_kernel, lds);
  if (rc_lds != RBX_OK) return rc_lds;
  hipLaunchKernelGGL(cm_bwd_kernel, dim3(static_cast<unsigned>((batch + kCmTile - 1) / kCmTile)), dim3(kCmBlock), lds, s, a);
  int rc2 = check_launch("crossmix_bwd");
  if (rc2 != RBX_OK) return rc2;
  int chunks;
  XtyArgs x{};
  x.part = part; x.B = batch;
  cm_split(batch, &chunks, &x.rpc);
  // dU[e, m, j] = sum_b (dout x0)[b, m] (p_e h2_e)[b, j]
  x.A = d_dout; x.lda = dout_stride; x.A2 = d_x0; x.lda2 = x0_stride; x.Bm = a.ph2; x.ldb = ER; x.I = n; x.J = ER;
  if ((rc2 = cm_xty(s, x, 1, chunks, r, 0, d_du)) != RBX_OK) return rc2;
  // db[m] = sum_b (dout x0)[b, m]
  x.Bm = nullptr; x.J = 1;
  if ((rc2 = cm_xty(s, x, 1, chunks, 0, 0, d_db)) != RBX_OK) return rc2;
  // dV[e, m, j] = sum_b x_l[b, m] da1_e[b, j]
  x.A = d_xl; x.lda = xl_stride; x.A2 = nullptr; x.Bm = a.da1; x.ldb = ER; x.J = ER;
  if ((rc2 = cm_xty(s, x, 1, chunks, r, 0, d_dv)) != RBX_OK) return rc2;
  // dG[e, m] (+)= sum_b dz[b, e] x_l[b, m]
  x.A = a.dz; x.lda = E; x.Bm = d_xl; x.ldb = xl_stride; x.I = E; x.J = n;
  if ((rc2 = cm_xty(s, x, 1, chunks, 0, accumulate, d_dg)) != RBX_OK) return rc2;
  // dC[e, i, j] = sum_b da2_e[b, i] h1_e[b, j]
  x.A = a.da2; x.lda = ER; x.az = r; x.Bm = a.h1; x.ldb = ER; x.bz = r; x.I = r; x.J = r;
  return cm_xty(s, x, E, chunks, 0, 0, d_dc);
}
