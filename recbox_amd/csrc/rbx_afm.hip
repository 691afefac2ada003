// rbx_afm.hip -- Attentional FM's pair-attention pooling (gfx950, wave64).  Replaces the ATen lines of RecBole's AFM
// (third_party/recbole/model/context_aware_recommender/afm.py:75-99 over AttLayer, model/layers.py:236-261), whose
// [B, P, D] pair products and [B, P, A] attention hidden layer are written, re-read and kept by autograd.  With x [B, F, D],
// W [A, D] (no bias), h [A] and the P = F (F - 1) / 2 pairs k = (i, j), i < j, in row-major order:
//   p_k = x_i * x_j     s_k = sum_a h_a relu(W p_k)_a     a = softmax_k(s)     out = sum_k a_k p_k
//
// Both kernels: a workgroup has 1, 2 or 4 wavefronts (as many as fit the LDS budget) and every wavefront owns ONE sample at a
// time: samples b = nw blockIdx.x + wave, + nw gridDim.x, ...  The sample's x [F, D] is staged in the wavefront's LDS once;
// the pairs are walked in tiles of 16.  The A operand of v_mfma_f32_16x16x4_f32 (exact fp32; rows = pairs, k = column of x,
// columns = attention units) is formed on the fly, xs[i][k] * xs[j][k], from a pair table in LDS; the wavefront's share of W
// sits in D / 4 x ceil(A / 16) B-operand registers for all its samples.  A and the last pair tile are padded with zeros.
//
// afm_fwd_kernel   per tile relu, the h product (in-lane over the unit blocks, then the 16 lanes by shuffles) -> 16 logits in
//                  LDS and a running maximum; then e = exp(s - max), the sum, a = e / sum as an IEEE division (one pair gives
//                  exactly 1, P equal logits exactly 1.0f / P) and out = sum_k a_k p_k, 64 / D lane groups added in order.
//                  Writes out [B, D], the statistics (max, sum) [2, B] and, when asked, attn [B, P].
// afm_bwd_kernel   recomputes the logits tile by tile with the forward's instructions (the same bits), a_k from the saved
//                  statistics, g_k = dout . p_k, ds_k = a_k (g_k - dout . out), dpre = ds_k h [pre > 0].  dW += dpre^T p runs
//                  on the MFMA with k = pair straight from the accumulator layout and stays in accumulators across all samples
//                  of the wavefront; dp = a_k dout + dpre W is a second chain over k = unit (dpre through a [A][16] LDS image,
//                  W from LDS); dx_i += dp * x_j, dx_j += dp * x_i are added in LDS, one lane per column walking the tile's
//                  pairs in order, and dx [F, D] is written once per sample.  Each wavefront writes one row (dW, dh) of the
//                  workspace; afm_tail_kernel adds the rows in a fixed order.
// No atomics, every sum in a fixed order: two runs give the same bits.  No host read-back, nothing allocated; everything on
// the caller's stream.  Nothing of B P D or B P A elements exists.
#include "rbx_internal.h"
#include "rbx_tile16.h"

namespace rbx {

constexpr int kAfMinF = 2, kAfMaxF = 39;
constexpr int kAfMinD = 4, kAfMaxD = 64;
constexpr int kAfMaxA = 64;
constexpr int kAfTile = 16;                 // pairs per tile = rows of the MFMA
constexpr int kAfMaxGrid = 512;             // workgroups of a launch; x up to 4 wavefronts = rows of the workspace
constexpr int kAfLdsBytes = 64 * 1024;      // dynamic LDS a workgroup may take

struct AfmArgs {
  const float* x;        // x[b xsb + f xsf + d]
  long long xsb, xsf;
  const float* w;        // [A, D]
  const float* h;        // [A]
  const float* dout;     // backward: dout[b dsb + d]
  long long dsb;
  const float* out_in;   // backward: out [B, D]
  const float* stat_in;  // backward: [2, B]
  float* out;            // forward: [B, D]
  float* stat;           // forward: [2, B]
  float* attn;           // forward: [B, P] or NULL
  float* dx;             // backward: [B, F, D] or NULL
  float* part;           // backward: [rows, A D + A]
  long long B;
  int F, D, A, P, want_dw;
};

// unit / column blocks the kernels are instantiated for: 1, 2 or 4 blocks of 16
static __host__ __device__ inline int af_blocks(int n) { return n <= 16 ? 1 : (n <= 32 ? 2 : 4); }
// row stride of W [A, D] in LDS: the four quads of a B operand read rows 4 s + quad, 16 floats each, in distinct banks
static __host__ __device__ inline int af_ldd(int nd) { return (nd & 1) ? 16 * nd : 16 * nd + 16; }
static __host__ __device__ inline int af_fwd_wave_floats(int F, int D) { return F * D + pad16(F * (F - 1) / 2) + 64; }
static __host__ __device__ inline int af_bwd_wave_floats(int F, int D, int na, int nd) {
  return 2 * F * D + 16 * 16 * (na > nd ? na : nd) + 64;
}
static __host__ __device__ inline int af_fwd_shared_floats(int F) { return pad16(F * (F - 1) / 2) / 2; }
static __host__ __device__ inline int af_bwd_shared_floats(int F, int na, int nd) {
  return pad16(F * (F - 1) / 2) / 2 + 16 * na * af_ldd(nd);
}
static int af_waves(int shared_floats, int wave_floats) {
  for (int nw = 4; nw > 1; nw >>= 1)
    if (4LL * (shared_floats + static_cast<long long>(nw) * wave_floats) <= kAfLdsBytes) return nw;
  return 1;
}
static int af_bwd_waves(int F, int D, int A) {
  const int na = af_blocks(A), nd = af_blocks(D);
  return af_waves(af_bwd_shared_floats(F, na, nd), af_bwd_wave_floats(F, D, na, nd));
}
static unsigned af_grid(int64_t batch, int nw) {
  const int64_t need = (batch + nw - 1) / nw;
  return static_cast<unsigned>(need < kAfMaxGrid ? need : kAfMaxGrid);
}

// sum over the 16 lanes that share a quad

// the pair table: entry k = i | j << 8 of pair k in row-major order, 0 beyond P
__device__ __forceinline__ void af_pairs(unsigned short* pij, const int F, const int P, const int ppad) {
  for (int k = P + threadIdx.x; k < ppad; k += blockDim.x) pij[k] = 0;
  for (int i = threadIdx.x; i < F - 1; i += blockDim.x) {
    const int k0 = i * (2 * F - i - 1) / 2;
    for (int j = i + 1; j < F; ++j) pij[k0 + j - i - 1] = static_cast<unsigned short>(i | (j << 8));
  }
}

// x[b] [F, D] into xs (zeros when the sample does not exist): one wavefront, float4 lanes
__device__ __forceinline__ void af_stage(const AfmArgs& g, const long long b, const bool ok, const int lane, float* xs) {
  const int d4 = g.D >> 2, n = g.F * d4;
  for (int idx = lane; idx < n; idx += 64) {
    const int f = idx / d4, q = idx - f * d4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ok) v = *reinterpret_cast<const float4*>(g.x + b * g.xsb + f * g.xsf + 4 * q);
    *reinterpret_cast<float4*>(xs + 4 * idx) = v;
  }
}

// this lane's B operands of W p: wf[n][s] = W[16 n + col][4 s + quad], and its units' h
template <int NA, int KS>
__device__ __forceinline__ void af_load_w(const AfmArgs& g, const int col, const int quad, float (&wf)[NA][KS], float (&hr)[NA]) {
  const int nkd = g.D >> 2;
#pragma unroll
  for (int n = 0; n < NA; ++n) {
    const int u = 16 * n + col;
#pragma unroll
    for (int s = 0; s < KS; ++s) wf[n][s] = (u < g.A && s < nkd) ? g.w[u * g.D + 4 * s + quad] : 0.f;
    hr[n] = u < g.A ? g.h[u] : 0.f;
  }
}

// pre-activations of pair tile t (acc[n][r]: unit 16 n + col, pair 16 t + 4 quad + r) and the four logits of this quad's
// pairs (the same value in its 16 lanes).  Forward and backward call this: the same instructions, the same bits.
template <int NA, int KS>
__device__ __forceinline__ void af_tile_logits(const float* xs, const unsigned short* pij, const int t, const int P, const int D,
                                               const int col, const int quad, const float (&wf)[NA][KS], const float (&hr)[NA],
                                               f32x4 (&acc)[NA], float (&lg)[4]) {
  const int k = kAfTile * t + col, nkd = D >> 2;
  const unsigned ij = pij[k];
  const float* xi = xs + (ij & 255u) * D + quad;
  const float* xj = xs + (ij >> 8) * D + quad;
  const bool valid = k < P;
#pragma unroll
  for (int n = 0; n < NA; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    if (s < nkd) {
      const float a = valid ? xi[4 * s] * xj[4 * s] : 0.f;
#pragma unroll
      for (int n = 0; n < NA; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, wf[n][s], acc[n], 0, 0, 0);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float v = 0.f;
#pragma unroll
    for (int n = 0; n < NA; ++n) v = fma_rn(hr[n], fmaxf(acc[n][r], 0.f), v);
    lg[r] = group_sum<16, kWave>(v);
  }
}

extern __shared__ __attribute__((aligned(16))) float af_smem[];

template <int NA, int ND>
__global__ __launch_bounds__(256) void afm_fwd_kernel(const AfmArgs g) {
  constexpr int KS = 4 * ND;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, col = lane & 15, quad = lane >> 4, nw = blockDim.x >> 6;
  const int F = g.F, D = g.D, P = g.P, FD = F * D, ppad = pad16(P);
  unsigned short* pij = reinterpret_cast<unsigned short*>(af_smem);
  float* xs = af_smem + af_fwd_shared_floats(F) + wv * af_fwd_wave_floats(F, D);   // [F, D]
  float* lgs = xs + FD;                                                            // [ppad] logits, then e, then a
  float* red = lgs + ppad;                                                         // [64 / D][D] partial sums of out
  af_pairs(pij, F, P, ppad);
  float wf[NA][KS], hr[NA];
  af_load_w<NA, KS>(g, col, quad, wf, hr);
  const int ntile = ppad / kAfTile;
  const int G = 64 / D, gi = lane / D, c = lane - gi * D;

  const long long step = static_cast<long long>(gridDim.x) * nw;
  for (long long b0 = static_cast<long long>(blockIdx.x) * nw; b0 < g.B; b0 += step) {      // uniform over the workgroup
    const long long b = b0 + wv;
    const bool ok = b < g.B;
    af_stage(g, b, ok, lane, xs);
    __syncthreads();                       // xs (and, the first time, the pair table)
    float m = -INFINITY;
    for (int t = 0; t < ntile; ++t) {
      f32x4 acc[NA];
      float lg[4];
      af_tile_logits<NA, KS>(xs, pij, t, P, D, col, quad, wf, hr, acc, lg);
      const int k0 = kAfTile * t + 4 * quad;
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (k0 + r < P) m = fmaxf(m, lg[r]);
      if (col == 0) *reinterpret_cast<float4*>(lgs + k0) = make_float4(lg[0], lg[1], lg[2], lg[3]);
    }
    m = fmaxf(m, __shfl_xor(m, 16, 64));
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    __syncthreads();                       // the logits
    float sum = 0.f;
    for (int k = lane; k < P; k += 64) {
      const float e = expf(lgs[k] - m);
      lgs[k] = e;
      sum += e;
    }
    sum = group_sum<64>(sum);
    if (ok && lane == 0) {
      g.stat[b] = m;
      g.stat[g.B + b] = sum;
    }
    for (int k = lane; k < P; k += 64) {   // the entries this lane wrote
      const float a = lgs[k] / sum;
      lgs[k] = a;
      if (g.attn != nullptr && ok) g.attn[b * P + k] = a;
    }
    __syncthreads();                       // a
    if (gi < G) {
      float o = 0.f;
      for (int k = gi; k < P; k += G) {
        const unsigned ij = pij[k];
        o = fma_rn(lgs[k], mul_rn(xs[(ij & 255u) * D + c], xs[(ij >> 8) * D + c]), o);
      }
      red[gi * D + c] = o;
    }
    __syncthreads();
    if (lane < D) {
      float o = red[lane];
      for (int q = 1; q < G; ++q) o += red[q * D + lane];
      if (ok) g.out[b * D + lane] = o;
    }
    __syncthreads();                       // xs, lgs and red are written again for the next sample
  }
}

template <int NA, int ND>
__global__ __launch_bounds__(256) void afm_bwd_kernel(const AfmArgs g) {
  constexpr int KS = 4 * ND, DP = 16 * ND, MX = 16 * (NA > ND ? NA : ND);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, col = lane & 15, quad = lane >> 4, nw = blockDim.x >> 6;
  const int F = g.F, D = g.D, A = g.A, P = g.P, FD = F * D, ppad = pad16(P), ldd = af_ldd(ND), nka = (A + 3) >> 2;
  unsigned short* pij = reinterpret_cast<unsigned short*>(af_smem);
  float* wl = af_smem + ppad / 2;                                                  // W [16 NA][ldd], zero padded
  float* xs = af_smem + af_bwd_shared_floats(F, NA, ND) + wv * af_bwd_wave_floats(F, D, NA, ND);   // [F, D]
  float* dxs = xs + FD;                                                            // [F, D]
  float* dpw = dxs + FD;                   // dpre of the tile [16 NA][16]; afterwards dp of the tile [16][DP]
  float* dd = dpw + 16 * MX;               // dout[b], zeros beyond D  [64]
  af_pairs(pij, F, P, ppad);
  for (int i = threadIdx.x; i < 16 * NA * ldd; i += blockDim.x) {
    const int u = i / ldd, d = i - u * ldd;
    wl[i] = (u < A && d < D) ? g.w[u * D + d] : 0.f;
  }
  float wf[NA][KS], hr[NA];
  af_load_w<NA, KS>(g, col, quad, wf, hr);
  const int ntile = ppad / kAfTile;

  f32x4 dwacc[NA][ND];                  // dW[16 n + 4 quad + r][16 m + col] over all samples of this wavefront
  float dh_acc[NA];                        // dh[16 n + col], this quad's pairs
#pragma unroll
  for (int n = 0; n < NA; ++n) {
    dh_acc[n] = 0.f;
#pragma unroll
    for (int mm = 0; mm < ND; ++mm) dwacc[n][mm] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  const long long step = static_cast<long long>(gridDim.x) * nw;
  for (long long b0 = static_cast<long long>(blockIdx.x) * nw; b0 < g.B; b0 += step) {      // uniform over the workgroup
    const long long b = b0 + wv;
    const bool ok = b < g.B;
    af_stage(g, b, ok, lane, xs);
    for (int i = lane; i < FD / 4; i += 64) *reinterpret_cast<float4*>(dxs + 4 * i) = make_float4(0.f, 0.f, 0.f, 0.f);
    dd[lane] = (ok && lane < D) ? g.dout[b * g.dsb + lane] : 0.f;
    __syncthreads();                       // xs, dxs, dd (and, the first time, the pair table and W)
    // Gd = dout . out, summed exactly as g_k = dout . p_k below (this lane's columns col, col + 16, .., then the 16 lanes):
    // with one pair, out = p_0 and ds cancels to the bit
    float Gd;
    {
      float p = 0.f;
      for (int cc = col; cc < D; cc += 16) p = fma_rn(dd[cc], ok ? g.out_in[b * D + cc] : 0.f, p);
      Gd = group_sum<16, kWave>(p);
    }
    const float m = ok ? g.stat_in[b] : 0.f, sum = ok ? g.stat_in[g.B + b] : 1.f;

    for (int t = 0; t < ntile; ++t) {
      f32x4 acc[NA];
      float lg[4], ar[4], dpr[NA][4];
      unsigned ijr[4];
      af_tile_logits<NA, KS>(xs, pij, t, P, D, col, quad, wf, hr, acc, lg);
      const int k0 = kAfTile * t + 4 * quad;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool valid = k0 + r < P;
        const unsigned ij = pij[k0 + r];
        ijr[r] = ij;
        const float* xi = xs + (ij & 255u) * D;
        const float* xj = xs + (ij >> 8) * D;
        float p = 0.f;
        for (int cc = col; cc < D; cc += 16) p = fma_rn(dd[cc], mul_rn(xi[cc], xj[cc]), p);
        const float gk = group_sum<16, kWave>(p);
        const float a = valid ? expf(lg[r] - m) / sum : 0.f;
        const float ds = a * (gk - Gd);
        ar[r] = a;
#pragma unroll
        for (int n = 0; n < NA; ++n) {
          const float pre = acc[n][r];
          dh_acc[n] = fma_rn(ds, fmaxf(pre, 0.f), dh_acc[n]);
          dpr[n][r] = pre > 0.f ? ds * hr[n] : 0.f;
        }
      }
      if (g.want_dw) {                     // dW += dpre^T p: k-step r takes the pairs 4 quad + r, as the accumulators hold them
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool valid = k0 + r < P;
          const float* xi = xs + (ijr[r] & 255u) * D;
          const float* xj = xs + (ijr[r] >> 8) * D;
#pragma unroll
          for (int mm = 0; mm < ND; ++mm) {
            const int cc = 16 * mm + col;
            const float bv = (valid && cc < D) ? mul_rn(xi[cc], xj[cc]) : 0.f;
#pragma unroll
            for (int n = 0; n < NA; ++n) dwacc[n][mm] = __builtin_amdgcn_mfma_f32_16x16x4f32(dpr[n][r], bv, dwacc[n][mm], 0, 0, 0);
          }
        }
      }
#pragma unroll
      for (int n = 0; n < NA; ++n)
        *reinterpret_cast<float4*>(dpw + (16 * n + col) * 16 + 4 * quad) = make_float4(dpr[n][0], dpr[n][1], dpr[n][2], dpr[n][3]);
      __syncthreads();                     // dpre of the tile
      f32x4 dpacc[ND];                  // dp: pair 4 quad + r, column 16 m + col
#pragma unroll
      for (int mm = 0; mm < ND; ++mm) {
        const float dj = dd[16 * mm + col];
        dpacc[mm] = f32x4{ar[0] * dj, ar[1] * dj, ar[2] * dj, ar[3] * dj};
      }
#pragma unroll
      for (int s = 0; s < 4 * NA; ++s) {
        if (s < nka) {
          const float av = dpw[64 * s + lane];                                     // dpre[unit 4 s + quad][pair col]
#pragma unroll
          for (int mm = 0; mm < ND; ++mm)
            dpacc[mm] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, wl[(4 * s + quad) * ldd + 16 * mm + col], dpacc[mm], 0, 0, 0);
        }
      }
      __syncthreads();                     // dpre is read; the buffer takes dp [16][DP]
#pragma unroll
      for (int mm = 0; mm < ND; ++mm)
#pragma unroll
        for (int r = 0; r < 4; ++r) dpw[(4 * quad + r) * DP + 16 * mm + col] = dpacc[mm][r];
      __syncthreads();
      if (lane < D) {                      // one lane per column walks the tile's pairs in order
        const int kn = (P - kAfTile * t) < kAfTile ? (P - kAfTile * t) : kAfTile;
        for (int q = 0; q < kn; ++q) {
          const unsigned ij = pij[kAfTile * t + q];
          const int oi = (ij & 255u) * D + lane, oj = (ij >> 8) * D + lane;
          const float v = dpw[q * DP + lane];
          dxs[oi] = fma_rn(v, xs[oj], dxs[oi]);
          dxs[oj] = fma_rn(v, xs[oi], dxs[oj]);
        }
      }
      __syncthreads();                     // dpw is written again by the next tile
    }
    if (g.dx != nullptr && ok) {
      float* dxb = g.dx + b * FD;
      for (int i = lane; i < FD / 4; i += 64) *reinterpret_cast<float4*>(dxb + 4 * i) = *reinterpret_cast<const float4*>(dxs + 4 * i);
    }
    __syncthreads();                       // xs, dxs and dd are written again for the next sample
  }

  const long long rl = static_cast<long long>(A) * D + A;
  float* row = g.part + (static_cast<long long>(blockIdx.x) * nw + wv) * rl;
  if (g.want_dw) {
#pragma unroll
    for (int n = 0; n < NA; ++n)
#pragma unroll
      for (int mm = 0; mm < ND; ++mm)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int u = 16 * n + 4 * quad + r, cc = 16 * mm + col;
          if (u < A && cc < D) row[u * D + cc] = dwacc[n][mm][r];
        }
  }
#pragma unroll
  for (int n = 0; n < NA; ++n) {
    float v = dh_acc[n];
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    if (quad == 0 && 16 * n + col < A) row[static_cast<long long>(A) * D + 16 * n + col] = v;
  }
}

// dW[e] / dh[e - A D] = sum over the rows of the workspace, in colsum16's order
__global__ __launch_bounds__(256) void afm_tail_kernel(const float* __restrict__ part, const int rows, const int rl, const int ad,
                                                       float* __restrict__ dw, float* __restrict__ dh) {
  __shared__ float sm[16][17];
  const int c = threadIdx.x & 15, r = threadIdx.x >> 4, e = blockIdx.x * 16 + c;
  colsum16(part, rows, rl, e, r, c, sm);
  if (r == 0 && e < rl) {
    if (e < ad) {
      if (dw != nullptr) dw[e] = sm[0][c];
    } else if (dh != nullptr) {
      dh[e - ad] = sm[0][c];
    }
  }
}

static int af_check(const char* what, int64_t batch, int32_t n_fields, int32_t dim, int32_t att_dim, int32_t dtype, const void* x,
                    int64_t xs_b, int64_t xs_f) {
  if (batch < 0) return fail(RBX_ERR_INVALID, "%s: batch=%lld", what, static_cast<long long>(batch));
  if (!rbx_afm_supported(n_fields, dim, att_dim))
    return fail(RBX_ERR_UNSUPPORTED, "%s: n_fields=%d in [%d,%d], dim=%d a multiple of 4 in [%d,%d], att_dim=%d in [1,%d]", what,
                n_fields, kAfMinF, kAfMaxF, dim, kAfMinD, kAfMaxD, att_dim, kAfMaxA);
  if (dtype != RBX_F32) return fail(RBX_ERR_UNSUPPORTED, "%s: tensor dtype code %d (float32 only)", what, dtype);
  if (x != nullptr && (!aligned16(x) || (xs_b & 3) != 0 || (xs_f & 3) != 0 || xs_f < dim || xs_b < 0))
    return fail(RBX_ERR_UNSUPPORTED, "%s: x must be 16-byte aligned with strides that are multiples of 4 floats", what);
  return RBX_OK;
}

}  // namespace rbx

extern "C" int rbx_afm_supported(int32_t n_fields, int32_t dim, int32_t att_dim) {
  using namespace rbx;
  return n_fields >= kAfMinF && n_fields <= kAfMaxF && dim >= kAfMinD && dim <= kAfMaxD && (dim & 3) == 0 && att_dim >= 1 &&
         att_dim <= kAfMaxA;
}

#define RBX_AF_LAUNCH(KERNEL, NA_, ND_) hipLaunchKernelGGL((KERNEL<NA_, ND_>), grid, block, lds, s, args)
#define RBX_AF_ROW(KERNEL, NA_)                                  \
  do {                                                           \
    if (nd == 1) RBX_AF_LAUNCH(KERNEL, NA_, 1);                  \
    else if (nd == 2) RBX_AF_LAUNCH(KERNEL, NA_, 2);             \
    else RBX_AF_LAUNCH(KERNEL, NA_, 4);                          \
  } while (0)
#define RBX_AF_DISPATCH(KERNEL)                                  \
  do {                                                           \
    if (na == 1) RBX_AF_ROW(KERNEL, 1);                          \
    else if (na == 2) RBX_AF_ROW(KERNEL, 2);                     \
    else RBX_AF_ROW(KERNEL, 4);                                  \
  } while (0)

extern "C" int rbx_afm_fwd(const float* d_x, int64_t x_stride_b, int64_t x_stride_f, const float* d_w, const float* d_h,
                           int64_t batch, int32_t n_fields, int32_t dim, int32_t att_dim, int32_t dtype, float* d_out,
                           float* d_stat, float* d_attn, void* stream) {
  using namespace rbx;
  const int rc = af_check("afm_fwd", batch, n_fields, dim, att_dim, dtype, d_x, x_stride_b, x_stride_f);
  if (rc != RBX_OK) return rc;
  if (batch == 0) return RBX_OK;
  if (!d_x || !d_w || !d_h || !d_out || !d_stat) return fail(RBX_ERR_INVALID, "afm_fwd: NULL tensor");
  AfmArgs args = {};
  args.x = d_x; args.xsb = x_stride_b; args.xsf = x_stride_f; args.w = d_w; args.h = d_h;
  args.out = d_out; args.stat = d_stat; args.attn = d_attn;
  args.B = batch; args.F = n_fields; args.D = dim; args.A = att_dim; args.P = n_fields * (n_fields - 1) / 2;
  const int na = af_blocks(att_dim), nd = af_blocks(dim);
  const int shared = af_fwd_shared_floats(n_fields), wave = af_fwd_wave_floats(n_fields, dim);
  const int nw = af_waves(shared, wave);
  const size_t lds = 4 * (static_cast<size_t>(shared) + static_cast<size_t>(nw) * wave);
  if (lds > static_cast<size_t>(kAfLdsBytes)) return fail(RBX_ERR_UNSUPPORTED, "afm_fwd: %zu bytes of LDS", lds);
  const dim3 grid(af_grid(batch, nw)), block(64 * nw);
  hipStream_t s = as_stream(stream);
  RBX_AF_DISPATCH(afm_fwd_kernel);
  return check_launch("afm_fwd");
}

extern "C" size_t rbx_afm_bwd_workspace_size(int64_t batch, int32_t n_fields, int32_t dim, int32_t att_dim) {
  using namespace rbx;
  if (batch <= 0 || !rbx_afm_supported(n_fields, dim, att_dim)) return 0;
  const int nw = af_bwd_waves(n_fields, dim, att_dim);
  return static_cast<size_t>(af_grid(batch, nw)) * nw * (static_cast<size_t>(att_dim) * dim + att_dim) * sizeof(float);
}

extern "C" int rbx_afm_bwd(const float* d_dout, int64_t dout_stride_b, const float* d_x, int64_t x_stride_b, int64_t x_stride_f,
                           const float* d_w, const float* d_h, const float* d_out, const float* d_stat, int64_t batch,
                           int32_t n_fields, int32_t dim, int32_t att_dim, int32_t dtype, float* d_dx, float* d_dw, float* d_dh,
                           void* d_workspace, size_t workspace_bytes, void* stream) {
  using namespace rbx;
  const int rc = af_check("afm_bwd", batch, n_fields, dim, att_dim, dtype, d_x, x_stride_b, x_stride_f);
  if (rc != RBX_OK) return rc;
  if (batch == 0) return RBX_OK;
  if (!d_dout || !d_x || !d_w || !d_h || !d_out || !d_stat) return fail(RBX_ERR_INVALID, "afm_bwd: NULL tensor");
  if (!aligned16(d_dout) || (dout_stride_b & 3) != 0 || dout_stride_b < dim)
    return fail(RBX_ERR_UNSUPPORTED, "afm_bwd: d_dout must be 16-byte aligned with a row stride that is a multiple of 4 floats");
  if (d_workspace == nullptr || workspace_bytes < rbx_afm_bwd_workspace_size(batch, n_fields, dim, att_dim))
    return fail(RBX_ERR_WORKSPACE, "afm_bwd: workspace too small");
  AfmArgs args = {};
  args.x = d_x; args.xsb = x_stride_b; args.xsf = x_stride_f; args.w = d_w; args.h = d_h;
  args.dout = d_dout; args.dsb = dout_stride_b; args.out_in = d_out; args.stat_in = d_stat;
  args.dx = d_dx; args.part = static_cast<float*>(d_workspace);
  args.B = batch; args.F = n_fields; args.D = dim; args.A = att_dim; args.P = n_fields * (n_fields - 1) / 2;
  args.want_dw = d_dw != nullptr;
  const int na = af_blocks(att_dim), nd = af_blocks(dim);
  const int shared = af_bwd_shared_floats(n_fields, na, nd), wave = af_bwd_wave_floats(n_fields, dim, na, nd);
  const int nw = af_bwd_waves(n_fields, dim, att_dim);
  const size_t lds = 4 * (static_cast<size_t>(shared) + static_cast<size_t>(nw) * wave);
  if (lds > static_cast<size_t>(kAfLdsBytes)) return fail(RBX_ERR_UNSUPPORTED, "afm_bwd: %zu bytes of LDS", lds);
  const dim3 grid(af_grid(batch, nw)), block(64 * nw);
  hipStream_t s = as_stream(stream);
  RBX_AF_DISPATCH(afm_bwd_kernel);
  if (d_dw != nullptr || d_dh != nullptr) {
    const int rl = att_dim * dim + att_dim;
    hipLaunchKernelGGL(afm_tail_kernel, dim3((rl + 15) / 16), dim3(256), 0, s, args.part, static_cast<int>(grid.x) * nw, rl,
                       att_dim * dim, d_dw, d_dh);
  }
  return check_launch("afm_bwd");
}
#undef RBX_AF_DISPATCH
#undef RBX_AF_ROW
#undef RBX_AF_LAUNCH
