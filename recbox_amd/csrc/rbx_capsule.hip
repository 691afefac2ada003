// rbx_capsule.hip -- SURVEY f-4: dynamic routing of the multi-interest matching models (gfx950, wave64).  Replaces rechub's
// CapsuleNetwork (third_party/rechub/basic/layers.py:553-648) under MIND (bilinear_type 0) and ComirecDR (bilinear_type 2).
//
//   hat      hat[b, l, k D + e] = sum_d W[l, k D + e, d] x[b, l, d]      (layers.py:595-596, whose product is [B, L, K D, D]):
//            one GEMM per position l on the fp32 MFMA (v_mfma_f32_32x32x2_f32: exact fp32 products and accumulation).
//   route    per (b, k): softmax over l of the logits, masked positions set to 0 (no renormalisation), s = sum_l c[l] hat[l],
//            v = squash(s), logits += hat v; `updates` of those and one output iteration (layers.py:620-641) with the task's
//            [L, D] slice of hat in LDS: hat is read once.
//   bwd      gradients flow through the output iteration only (stop_grad, layers.py:602-603): ds from dv and s, then
//            d_hat = c ds for the Linear forms, or for the bilinear form the two per-position GEMMs
//              dW[l, n, d] = sum_b c[b, k(n), l] ds[b, n] x[b, l, d]     dx[b, l, d] = sum_n c[b, k(n), l] ds[b, n] W[l, n, d]
//            whose [B, K D] operand is formed from c and ds between LDS and the MFMA: d_hat is never stored.
//
// capsule_hat_kernel    workgroup = (128 samples, position); x[:, l, :] of the tile sits k-major in LDS, W_l goes through LDS in
//                       slices of 64 of its K D rows; a wavefront owns 32 samples x 64 columns.
// capsule_route_kernel  wavefront = task (b, k), 1..4 tasks per workgroup; slab = [L][D + 1] (lane = position reads are
//                       conflict-free) + logits, c, mask [L] + v [D].  s is summed over l by the lane that owns the column, in
//                       order; the wave sums are butterflies: the same bits from run to run.
// capsule_ds_kernel     workgroup = sample: ds for its K rows, then (Linear forms) d_hat of the sample, summed over k in order
//                       for the shared form.
// capsule_dx_kernel     workgroup = (128 samples, position); n = K D is walked in slices of 32; wavefront = 32 samples x D.
// capsule_dw_kernel     workgroup = (position, 128 rows of n, split of kCapDwSplit samples); wavefront = 32 rows x D; partial
//                       sums to the workspace, capsule_reduce_kernel adds the splits in order (one split stores directly).
#include "rbx_internal.h"

namespace rbx {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kCapBM = 128;                // samples (or rows of n) per tile
constexpr int kCapLd = kCapBM + 2;         // LDS pitch of a k row of a [k, 128] operand
constexpr int kCapNC = 64;                 // rows of W_l per slice of the forward
constexpr int kCapKC = 32;                 // k per step of the backward GEMMs
constexpr int kCapMinDim = 4, kCapMaxDim = 128, kCapMaxK = 32;
constexpr int kCapDwSplit = 2048;          // samples per split of the dW reduction
constexpr int kCapSlabFloats = 14336;      // a routing task's LDS: L (D + 1) + 3 L + D floats at most (56 KiB)
constexpr int kCapWgFloats = 16000;        // LDS of a routing workgroup (under 64 KiB): 1..4 tasks

__device__ __forceinline__ int cap_acc_row(int r, int lk) { return (r & 3) + 8 * (r >> 2) + 4 * lk; }
__device__ __forceinline__ float4 cap_ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// ---- hat = W_l x_l ------------------------------------------------------------------------------------------------------
// dynamic LDS: Xs [D][130] | Ws [D][66]
__global__ __launch_bounds__(256) void capsule_hat_kernel(const float* __restrict__ X, const long long xs_b,
                                                          const long long xs_l, const float* __restrict__ W, const int B,
                                                          const int L, const int D, const int N, float* __restrict__ hat) {
  constexpr int LDW = kCapNC + 2;
  extern __shared__ float smem[];
  float* Xs = smem;
  float* Ws = Xs + D * kCapLd;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, li = lane & 31, lk = lane >> 5;
  const int l = blockIdx.y;
  const int b0 = static_cast<int>(blockIdx.x) * kCapBM;
  const int d4n = D >> 2;

  for (int i = tid; i < kCapBM * d4n; i += 256) {
    const int r = i / d4n, d = (i - r * d4n) * 4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (b0 + r < B) v = cap_ld4(X + (b0 + r) * xs_b + l * xs_l + d);
    Xs[(d + 0) * kCapLd + r] = v.x; Xs[(d + 1) * kCapLd + r] = v.y;
    Xs[(d + 2) * kCapLd + r] = v.z; Xs[(d + 3) * kCapLd + r] = v.w;
  }
  const float* Wl = W + static_cast<long long>(l) * N * D;
  for (int n0 = 0; n0 < N; n0 += kCapNC) {
    __syncthreads();                               // Xs is written; the previous slice's readers of Ws are done
    for (int i = tid; i < kCapNC * d4n; i += 256) {
      const int nn = i % kCapNC, d = (i / kCapNC) * 4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (n0 + nn < N) v = cap_ld4(Wl + static_cast<long long>(n0 + nn) * D + d);
      Ws[(d + 0) * LDW + nn] = v.x; Ws[(d + 1) * LDW + nn] = v.y;
      Ws[(d + 2) * LDW + nn] = v.z; Ws[(d + 3) * LDW + nn] = v.w;
    }
    __syncthreads();
    f32x16 acc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
    const float* xs = Xs + wv * 32 + li;
    const float* ws = Ws + li;
    for (int kk = 0; kk < D; kk += 2) {
      const float a = xs[(kk + lk) * kCapLd];
#pragma unroll
      for (int j = 0; j < 2; ++j)
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, ws[(kk + lk) * LDW + j * 32], acc[j], 0, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = n0 + j * 32 + li;
      if (col >= N) continue;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int b = b0 + wv * 32 + cap_acc_row(r, lk);
        if (b < B) hat[(static_cast<long long>(b) * L + l) * N + col] = acc[j][r];
      }
    }
  }
}

// ---- routing ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool cap_mask_on(const void* p, long long idx, int dt) {
  switch (dt) {
    case RBX_I32: return static_cast<const int*>(p)[idx] != 0;
    case RBX_I64: return static_cast<const long long*>(p)[idx] != 0;
    case RBX_F32: return static_cast<const float*>(p)[idx] != 0.f;
    default:      return static_cast<const unsigned char*>(p)[idx] != 0;
  }
}

// squash: f(n) = n / (1 + n) / sqrt(n + 1e-9), written as the reference writes it
__device__ __forceinline__ float cap_squash(float n) { return n / (1.f + n) / sqrtf(n + 1e-9f); }

// dynamic LDS: per task [L][D + 1] hat | logits [L] | c [L] | keep [L] | v [D]
__global__ void capsule_route_kernel(const float* __restrict__ hat, const long long hs_b, const long long hs_k,
                                     const long long hs_l, const void* __restrict__ mask, const int mask_dt,
                                     const long long ms_b, const long long ms_l, const float* __restrict__ init,
                                     const long long tasks, const int K, const int L, const int D, const int updates,
                                     const int slab, float* __restrict__ V, float* __restrict__ C, float* __restrict__ S) {
  extern __shared__ float smem[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int P = D + 1;
  float* hs = smem + static_cast<long long>(wv) * slab;
  float* lg = hs + L * P;
  float* cs = lg + L;
  float* keep = cs + L;
  float* vs = keep + L;
  const long long task = static_cast<long long>(blockIdx.x) * (blockDim.x >> 6) + wv;
  const bool live = task < tasks;
  const long long b = live ? task / K : 0;
  const int k = live ? static_cast<int>(task - b * K) : 0;

  if (live) {
    const float* src = hat + b * hs_b + k * hs_k;
    const int d4n = D >> 2;
    for (int i = lane; i < L * d4n; i += 64) {
      const int l = i / d4n, d = (i - l * d4n) * 4;
      const float4 v = cap_ld4(src + l * hs_l + d);
      float* dst = hs + l * P + d;
      dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
    }
    for (int l = lane; l < L; l += 64) {
      lg[l] = init != nullptr ? init[task * L + l] : 0.f;
      keep[l] = cap_mask_on(mask, b * ms_b + l * ms_l, mask_dt) ? 1.f : 0.f;
    }
  }
  __syncthreads();

  for (int it = 0; it <= updates; ++it) {
    // c = softmax over all L positions, then 0 at the masked ones
    float mx = -INFINITY;
    for (int l = lane; l < L; l += 64) mx = fmaxf(mx, lg[l]);
    mx = group_max<kWave>(mx);
    float sum = 0.f;
    for (int l = lane; l < L; l += 64) {
      const float e = expf(lg[l] - mx);
      cs[l] = e;
      sum += e;
    }
    sum = group_sum<64>(sum);
    for (int l = lane; l < L; l += 64) cs[l] = keep[l] != 0.f ? cs[l] / sum : 0.f;
    __syncthreads();
    // s = sum_l c[l] hat[l, :]: the lane that owns a column adds its L terms in order
    float sd[2] = {0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int d = lane + 64 * q;
      if (d < D)
        for (int l = 0; l < L; ++l) sd[q] = fma_rn(cs[l], hs[l * P + d], sd[q]);
    }
    const float n = group_sum<64>(sd[0] * sd[0] + sd[1] * sd[1]);
    const float f = cap_squash(n);
    const bool last = it == updates;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int d = lane + 64 * q;
      if (d < D) {
        const float v = f * sd[q];
        vs[d] = v;
        if (last && live) {
          V[task * D + d] = v;
          S[task * D + d] = sd[q];
        }
      }
    }
    if (last) {
      if (live)
        for (int l = lane; l < L; l += 64) C[task * L + l] = cs[l];
      break;
    }
    __syncthreads();
    // logits += hat v
    for (int l = lane; l < L; l += 64) {
      float dot = 0.f;
      for (int d = 0; d < D; ++d) dot = fma_rn(hs[l * P + d], vs[d], dot);
      lg[l] += dot;
    }
    __syncthreads();
  }
}

// ---- ds, and d_hat of the Linear forms ----------------------------------------------------------------------------------
// dynamic LDS: ds [K][D] | c [K][L]
__global__ __launch_bounds__(256) void capsule_ds_kernel(const float* __restrict__ dV, const float* __restrict__ S,
                                                         const float* __restrict__ C, const int K, const int L, const int D,
                                                         const int shared, float* __restrict__ dS, float* __restrict__ dHat) {
  extern __shared__ float smem[];
  float* dss = smem;
  float* cs = dss + K * D;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const long long b = blockIdx.x;
  for (int k = wv; k < K; k += 4) {
    const long long row = (b * K + k) * D;
    float s[2], g[2], nn = 0.f, dot = 0.f;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int d = lane + 64 * q;
      s[q] = d < D ? S[row + d] : 0.f;
      g[q] = d < D ? dV[row + d] : 0.f;
      nn += s[q] * s[q];
      dot += s[q] * g[q];
    }
    nn = group_sum<64>(nn);
    dot = group_sum<64>(dot);
    const float rs = 1.f / sqrtf(nn + 1e-9f);
    const float f = nn / (1.f + nn) * rs;
    // f'(n) = (n + eps)^-1/2 / (1 + n)^2 - n / (1 + n) (n + eps)^-3/2 / 2
    const float fp = rs / ((1.f + nn) * (1.f + nn)) - 0.5f * nn / (1.f + nn) * rs * rs * rs;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int d = lane + 64 * q;
      if (d < D) {
        const float v = f * g[q] + 2.f * fp * dot * s[q];
        dss[k * D + d] = v;
        if (dS != nullptr) dS[row + d] = v;
      }
    }
  }
  if (dHat == nullptr) return;
  for (int i = tid; i < K * L; i += 256) cs[i] = C[b * K * L + i];
  __syncthreads();
  const int d4n = D >> 2;
  if (shared != 0) {                               // d_hat [B, L, D] = sum_k c[b, k, l] ds[b, k, :], k in order
    float* dst = dHat + b * L * D;
    for (int i = tid; i < L * d4n; i += 256) {
      const int l = i / d4n, d = (i - l * d4n) * 4;
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int k = 0; k < K; ++k) {
        const float c = cs[k * L + l];
        const float4 g = *reinterpret_cast<const float4*>(dss + k * D + d);
        acc.x = fma_rn(c, g.x, acc.x); acc.y = fma_rn(c, g.y, acc.y);
        acc.z = fma_rn(c, g.z, acc.z); acc.w = fma_rn(c, g.w, acc.w);
      }
      *reinterpret_cast<float4*>(dst + static_cast<long long>(l) * D + d) = acc;
    }
  } else {                                         // d_hat [B, L, K D]
    const int n4n = K * d4n;
    float* dst = dHat + b * L * K * D;
    for (int i = tid; i < L * n4n; i += 256) {
      const int l = i / n4n, n = (i - l * n4n) * 4;
      const float c = cs[(n / D) * L + l];
      const float4 g = *reinterpret_cast<const float4*>(dss + n);
      *reinterpret_cast<float4*>(dst + static_cast<long long>(l) * K * D + n) = make_float4(c * g.x, c * g.y, c * g.z, c * g.w);
    }
  }
}

// ---- bilinear backward: dx ----------------------------------------------------------------------------------------------
// G[b, n] = g[b gs_b + l gs_l + n] (x c[b, n / D, l] when c is given).  dynamic LDS: Gs [32][130] | Ws [32][D] | Cs [K][128]
template <int NT>
__global__ __launch_bounds__(256) void capsule_dx_kernel(const float* __restrict__ W, const float* __restrict__ G,
                                                         const long long gs_b, const long long gs_l,
                                                         const float* __restrict__ C, const int B, const int L, const int D,
                                                         const int K, float* __restrict__ dX) {
  extern __shared__ float smem[];
  float* Gs = smem;
  float* Ws = Gs + kCapKC * kCapLd;
  float* Cs = Ws + kCapKC * D;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, li = lane & 31, lk = lane >> 5;
  const int l = blockIdx.y;
  const int b0 = static_cast<int>(blockIdx.x) * kCapBM;
  const int N = K * D, d4n = D >> 2;
  const float* Wl = W + static_cast<long long>(l) * N * D;

  for (int i = tid; i < K * kCapBM; i += 256) {
    const int k = i / kCapBM, r = i - k * kCapBM;
    Cs[i] = (C != nullptr) ? (b0 + r < B ? C[(static_cast<long long>(b0 + r) * K + k) * L + l] : 0.f) : 1.f;
  }
  f32x16 acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

  for (int n0 = 0; n0 < N; n0 += kCapKC) {
    __syncthreads();                               // Cs is written; the previous slice's readers are done
    for (int i = tid; i < kCapBM * (kCapKC / 4); i += 256) {
      const int r = i >> 3, n = n0 + (i & 7) * 4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (b0 + r < B && n < N) v = cap_ld4(G + (b0 + r) * gs_b + l * gs_l + n);
      float* dst = Gs + ((i & 7) * 4) * kCapLd + r;
      dst[0] = v.x; dst[kCapLd] = v.y; dst[2 * kCapLd] = v.z; dst[3 * kCapLd] = v.w;
    }
    for (int i = tid; i < kCapKC * d4n; i += 256) {
      const int nn = i / d4n, d = (i - nn * d4n) * 4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (n0 + nn < N) v = cap_ld4(Wl + static_cast<long long>(n0 + nn) * D + d);
      *reinterpret_cast<float4*>(Ws + nn * D + d) = v;
    }
    __syncthreads();
    const int row = wv * 32 + li;
#pragma unroll 4
    for (int kk = 0; kk < kCapKC; kk += 2) {
      const int n = n0 + kk + lk;
      const int k = n < N ? n / D : 0;
      const float a = Gs[(kk + lk) * kCapLd + row] * Cs[k * kCapBM + row];    // the c ds operand, formed here
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int col = j * 32 + li;
        const float w = col < D ? Ws[(kk + lk) * D + col] : 0.f;
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, w, acc[j], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int col = j * 32 + li;
    if (col >= D) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int b = b0 + wv * 32 + cap_acc_row(r, lk);
      if (b < B) dX[(static_cast<long long>(b) * L + l) * D + col] = acc[j][r];
    }
  }
}

// ---- bilinear backward: dW ----------------------------------------------------------------------------------------------
// out [split][L][N][D] (or dW itself with one split).  dynamic LDS: Gs [32][128] | Xs [32][D] | Cs [32][K]
template <int NT>
__global__ __launch_bounds__(256) void capsule_dw_kernel(const float* __restrict__ X, const long long xs_b,
                                                         const long long xs_l, const float* __restrict__ G,
                                                         const long long gs_b, const long long gs_l,
                                                         const float* __restrict__ C, const int B, const int L, const int D,
                                                         const int K, float* __restrict__ out) {
  extern __shared__ float smem[];
  float* Gs = smem;
  float* Xs = Gs + kCapKC * kCapBM;
  float* Cs = Xs + kCapKC * D;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, li = lane & 31, lk = lane >> 5;
  const int l = blockIdx.y;
  const int n0 = static_cast<int>(blockIdx.z) * kCapBM;
  const int b_begin = static_cast<int>(blockIdx.x) * kCapDwSplit;
  const int b_end = b_begin + kCapDwSplit < B ? b_begin + kCapDwSplit : B;
  const int N = K * D, d4n = D >> 2;
  const int my_n = n0 + wv * 32 + li;
  const int my_k = my_n < N ? my_n / D : 0;

  f32x16 acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

  for (int bb = b_begin; bb < b_end; bb += kCapKC) {
    __syncthreads();
    for (int i = tid; i < kCapKC * (kCapBM / 4); i += 256) {
      const int r = i >> 5, n = (i & 31) * 4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (bb + r < b_end && n0 + n < N) v = cap_ld4(G + (bb + r) * gs_b + l * gs_l + n0 + n);
      *reinterpret_cast<float4*>(Gs + r * kCapBM + n) = v;
    }
    for (int i = tid; i < kCapKC * d4n; i += 256) {
      const int r = i / d4n, d = (i - r * d4n) * 4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (bb + r < b_end) v = cap_ld4(X + (bb + r) * xs_b + l * xs_l + d);
      *reinterpret_cast<float4*>(Xs + r * D + d) = v;
    }
    for (int i = tid; i < kCapKC * K; i += 256) {
      const int r = i / K, k = i - r * K;
      Cs[i] = (C != nullptr) ? (bb + r < b_end ? C[(static_cast<long long>(bb + r) * K + k) * L + l] : 0.f) : 1.f;
    }
    __syncthreads();
#pragma unroll 4
    for (int kk = 0; kk < kCapKC; kk += 2) {
      const float a = Gs[(kk + lk) * kCapBM + wv * 32 + li] * Cs[(kk + lk) * K + my_k];    // the c ds operand, formed here
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int col = j * 32 + li;
        const float x = col < D ? Xs[(kk + lk) * D + col] : 0.f;
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, x, acc[j], 0, 0, 0);
      }
    }
  }
  float* mine = out + (static_cast<long long>(blockIdx.x) * L + l) * N * D;
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int col = j * 32 + li;
    if (col >= D) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int n = n0 + wv * 32 + cap_acc_row(r, lk);
      if (n < N) mine[static_cast<long long>(n) * D + col] = acc[j][r];
    }
  }
}

__global__ __launch_bounds__(256) void capsule_reduce_kernel(const float* __restrict__ part, const int splits,
                                                             const long long total, float* __restrict__ dW) {
  const long long j = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
  if (j >= total) return;
  float sum = 0.f;
  for (int s = 0; s < splits; ++s) sum += part[s * total + j];
  dW[j] = sum;
}

// ---- host -------------------------------------------------------------------------------------------------------------
static int cap_splits(int64_t batch) { return static_cast<int>((batch + kCapDwSplit - 1) / kCapDwSplit); }

static long long cap_slab(int L, int D) { return static_cast<long long>(L) * (D + 1) + 3LL * L + D; }

static int cap_check_shape(const char* what, int64_t batch, int32_t seq_len, int32_t dim, int32_t interests) {
  if (batch < 0) return fail(RBX_ERR_INVALID, "%s: batch=%lld", what, static_cast<long long>(batch));
  if (dim < kCapMinDim || dim > kCapMaxDim || (dim & 3) != 0)
    return fail(RBX_ERR_UNSUPPORTED, "%s: dim=%d is not a multiple of 4 in [%d,%d]", what, dim, kCapMinDim, kCapMaxDim);
  if (seq_len < 1 || seq_len > 65535) return fail(RBX_ERR_UNSUPPORTED, "%s: seq_len=%d", what, seq_len);
  if (interests < 1 || interests > kCapMaxK)
    return fail(RBX_ERR_UNSUPPORTED, "%s: interests=%d not in [1,%d]", what, interests, kCapMaxK);
  if (batch * static_cast<long long>(interests) > INT_MAX || batch * static_cast<long long>(seq_len) > INT_MAX)
    return fail(RBX_ERR_UNSUPPORTED, "%s: batch=%lld is too large", what, static_cast<long long>(batch));
  return RBX_OK;
}

template <int NT>
static int cap_launch_dx(const float* W, const float* G, long long gs_b, long long gs_l, const float* C, int B, int L, int D,
                         int K, float* dX, hipStream_t s) {
  const size_t lds = (static_cast<size_t>(kCapKC) * kCapLd + kCapKC * D + K * kCapBM) * sizeof(float);
  const int rc = allow_lds("capsule_bilinear_dx", &capsule_dx_kernel<NT>, lds);
  if (rc != RBX_OK) return rc;
  hipLaunchKernelGGL((capsule_dx_kernel<NT>), dim3((B + kCapBM - 1) / kCapBM, L), dim3(256), lds, s, W, G, gs_b, gs_l, C, B, L,
                     D, K, dX);
  return RBX_OK;
}

template <int NT>
static int cap_launch_dw(const float* X, long long xs_b, long long xs_l, const float* G, long long gs_b, long long gs_l,
                         const float* C, int B, int L, int D, int K, float* out, hipStream_t s) {
  const size_t lds = (static_cast<size_t>(kCapKC) * kCapBM + kCapKC * D + kCapKC * K) * sizeof(float);
  const int rc = allow_lds("capsule_bilinear_dw", &capsule_dw_kernel<NT>, lds);
  if (rc != RBX_OK) return rc;
  hipLaunchKernelGGL((capsule_dw_kernel<NT>), dim3(cap_splits(B), L, (K * D + kCapBM - 1) / kCapBM), dim3(256), lds, s, X, xs_b,
                     xs_l, G, gs_b, gs_l, C, B, L, D, K, out);
  return RBX_OK;
}

}  // namespace rbx

extern "C" int rbx_capsule_route_supported(int32_t seq_len, int32_t dim) {
  using namespace rbx;
  return seq_len >= 1 && dim >= kCapMinDim && dim <= kCapMaxDim && (dim & 3) == 0 && cap_slab(seq_len, dim) <= kCapSlabFloats;
}

extern "C" int32_t rbx_capsule_dw_split(void) { return rbx::kCapDwSplit; }

extern "C" int rbx_capsule_hat(const float* d_x, int64_t x_stride_b, int64_t x_stride_l, const float* d_w, int64_t batch,
                               int32_t seq_len, int32_t dim, int32_t interests, float* d_hat, void* stream) {
  using namespace rbx;
  int rc = cap_check_shape("capsule_hat", batch, seq_len, dim, interests);
  if (rc != RBX_OK) return rc;
  if (batch == 0) return RBX_OK;
  if (!d_x || !d_w || !d_hat) return fail(RBX_ERR_INVALID, "capsule_hat: NULL tensor");
  if (!aligned16(d_x) || !aligned16(d_w) || (x_stride_b & 3) != 0 || (x_stride_l & 3) != 0)
    return fail(RBX_ERR_UNSUPPORTED, "capsule_hat: bases must be 16-byte aligned and strides multiples of 4 floats");
  const int B = static_cast<int>(batch), N = interests * dim;
  const size_t lds = (static_cast<size_t>(dim) * kCapLd + dim * (kCapNC + 2)) * sizeof(float);
  rc = allow_lds("capsule_hat", &capsule_hat_kernel, lds);
  if (rc != RBX_OK) return rc;
  hipLaunchKernelGGL(capsule_hat_kernel, dim3((B + kCapBM - 1) / kCapBM, seq_len), dim3(256), lds, as_stream(stream), d_x,
                     x_stride_b, x_stride_l, d_w, B, seq_len, dim, N, d_hat);
  return check_launch("capsule_hat");
}

extern "C" int rbx_capsule_route_fwd(const float* d_hat, int64_t hat_stride_b, int64_t hat_stride_k, int64_t hat_stride_l,
                                     const void* d_mask, int32_t mask_dtype, int64_t mask_stride_b, int64_t mask_stride_l,
                                     const float* d_init, int64_t batch, int32_t interests, int32_t seq_len, int32_t dim,
                                     int32_t updates, float* d_v, float* d_c, float* d_s, void* stream) {
  using namespace rbx;
  int rc = cap_check_shape("capsule_route_fwd", batch, seq_len, dim, interests);
  if (rc != RBX_OK) return rc;
  if (!rbx_capsule_route_supported(seq_len, dim))
    return fail(RBX_ERR_UNSUPPORTED, "capsule_route_fwd: a [%d, %d] slice does not fit %d floats of LDS", seq_len, dim,
                kCapSlabFloats);
  if (updates < 0 || updates > 2) return fail(RBX_ERR_UNSUPPORTED, "capsule_route_fwd: updates=%d not in [0,2]", updates);
  if (mask_dtype != RBX_I32 && mask_dtype != RBX_I64 && mask_dtype != RBX_F32 && mask_dtype != RBX_MASK_U8)
    return fail(RBX_ERR_UNSUPPORTED, "capsule_route_fwd: mask_dtype=%d", mask_dtype);
  if (batch == 0) return RBX_OK;
  if (!d_hat || !d_mask || !d_v || !d_c || !d_s) return fail(RBX_ERR_INVALID, "capsule_route_fwd: NULL tensor");
  if (!aligned16(d_hat) || (hat_stride_b & 3) != 0 || (hat_stride_k & 3) != 0 || (hat_stride_l & 3) != 0)
    return fail(RBX_ERR_UNSUPPORTED, "capsule_route_fwd: hat must be 16-byte aligned with strides that are multiples of 4");
  const int slab = static_cast<int>(cap_slab(seq_len, dim));
  int per = kCapWgFloats / slab;
  per = per < 1 ? 1 : (per > 4 ? 4 : per);
  const long long tasks = batch * interests;
  const size_t lds = static_cast<size_t>(per) * slab * sizeof(float);
  hipLaunchKernelGGL(capsule_route_kernel, dim3(static_cast<unsigned>((tasks + per - 1) / per)), dim3(64 * per), lds,
                     as_stream(stream), d_hat, hat_stride_b, hat_stride_k, hat_stride_l, d_mask, mask_dtype, mask_stride_b,
                     mask_stride_l, d_init, tasks, interests, seq_len, dim, updates, slab, d_v, d_c, d_s);
  return check_launch("capsule_route_fwd");
}

extern "C" int rbx_capsule_route_bwd(const float* d_dv, const float* d_s, const float* d_c, int64_t batch, int32_t interests,
                                     int32_t seq_len, int32_t dim, int32_t shared, float* d_ds, float* d_dhat, void* stream) {
  using namespace rbx;
  int rc = cap_check_shape("capsule_route_bwd", batch, seq_len, dim, interests);
  if (rc != RBX_OK) return rc;
  const size_t lds = (static_cast<size_t>(interests) * dim + static_cast<size_t>(interests) * seq_len) * sizeof(float);
  if (lds > 64 * 1024) return fail(RBX_ERR_UNSUPPORTED, "capsule_route_bwd: interests * (dim + seq_len) = %zu floats", lds / 4);
  if (batch == 0) return RBX_OK;
  if (!d_dv || !d_s || (d_dhat != nullptr && !d_c) || (!d_ds && !d_dhat))
    return fail(RBX_ERR_INVALID, "capsule_route_bwd: NULL tensor");
  if (d_dhat != nullptr && !aligned16(d_dhat)) return fail(RBX_ERR_UNSUPPORTED, "capsule_route_bwd: dhat must be 16-byte aligned");
  hipLaunchKernelGGL(capsule_ds_kernel, dim3(static_cast<unsigned>(batch)), dim3(256), lds, as_stream(stream), d_dv, d_s, d_c,
                     interests, seq_len, dim, shared, d_ds, d_dhat);
  return check_launch("capsule_route_bwd");
}

extern "C" int rbx_capsule_bilinear_dx(const float* d_w, const float* d_g, int64_t g_stride_b, int64_t g_stride_l,
                                       const float* d_c, int64_t batch, int32_t seq_len, int32_t dim, int32_t interests,
                                       float* d_dx, void* stream) {
  using namespace rbx;
  int rc = cap_check_shape("capsule_bilinear_dx", batch, seq_len, dim, interests);
  if (rc != RBX_OK) return rc;
  if (batch == 0) return RBX_OK;
  if (!d_w || !d_g || !d_dx) return fail(RBX_ERR_INVALID, "capsule_bilinear_dx: NULL tensor");
  if (!aligned16(d_w) || !aligned16(d_g) || (g_stride_b & 3) != 0 || (g_stride_l & 3) != 0)
    return fail(RBX_ERR_UNSUPPORTED, "capsule_bilinear_dx: bases must be 16-byte aligned and strides multiples of 4 floats");
  const int B = static_cast<int>(batch);
  hipStream_t s = as_stream(stream);
  switch ((dim + 31) / 32) {
    case 1: rc = cap_launch_dx<1>(d_w, d_g, g_stride_b, g_stride_l, d_c, B, seq_len, dim, interests, d_dx, s); break;
    case 2: rc = cap_launch_dx<2>(d_w, d_g, g_stride_b, g_stride_l, d_c, B, seq_len, dim, interests, d_dx, s); break;
    case 3: rc = cap_launch_dx<3>(d_w, d_g, g_stride_b, g_stride_l, d_c, B, seq_len, dim, interests, d_dx, s); break;
    default: rc = cap_launch_dx<4>(d_w, d_g, g_stride_b, g_stride_l, d_c, B, seq_len, dim, interests, d_dx, s); break;
  }
  if (rc != RBX_OK) return rc;
  return check_launch("capsule_bilinear_dx");
}

extern "C" size_t rbx_capsule_bilinear_dw_workspace_size(int64_t batch, int32_t seq_len, int32_t dim, int32_t interests) {
  using namespace rbx;
  if (batch <= 0 || seq_len < 1 || dim < kCapMinDim || dim > kCapMaxDim || interests < 1 || interests > kCapMaxK) return 0;
  const int splits = cap_splits(batch);
  if (splits < 2) return 0;                        // one split stores dW directly
  const size_t per = static_cast<size_t>(seq_len) * interests * dim * dim * sizeof(float);
  return (splits * per + 255) / 256 * 256;
}

extern "C" int rbx_capsule_bilinear_dw(const float* d_x, int64_t x_stride_b, int64_t x_stride_l, const float* d_g,
                                       int64_t g_stride_b, int64_t g_stride_l, const float* d_c, int64_t batch,
                                       int32_t seq_len, int32_t dim, int32_t interests, float* d_dw, void* d_workspace,
                                       size_t workspace_bytes, void* stream) {
  using namespace rbx;
  int rc = cap_check_shape("capsule_bilinear_dw", batch, seq_len, dim, interests);
  if (rc != RBX_OK) return rc;
  if (!d_dw) return fail(RBX_ERR_INVALID, "capsule_bilinear_dw: NULL tensor");
  const long long total = static_cast<long long>(seq_len) * interests * dim * dim;
  hipStream_t s = as_stream(stream);
  if (batch == 0) {
    if (hipMemsetAsync(d_dw, 0, total * sizeof(float), s) != hipSuccess) return fail(RBX_ERR_LAUNCH, "capsule_bilinear_dw: memset");
    return RBX_OK;
  }
  if (!d_x || !d_g) return fail(RBX_ERR_INVALID, "capsule_bilinear_dw: NULL tensor");
  if (!aligned16(d_x) || !aligned16(d_g) || (x_stride_b & 3) != 0 || (x_stride_l & 3) != 0 || (g_stride_b & 3) != 0 ||
      (g_stride_l & 3) != 0)
    return fail(RBX_ERR_UNSUPPORTED, "capsule_bilinear_dw: bases must be 16-byte aligned and strides multiples of 4 floats");
  const int splits = cap_splits(batch);
  const size_t need = rbx_capsule_bilinear_dw_workspace_size(batch, seq_len, dim, interests);
  if (need > 0 && (d_workspace == nullptr || workspace_bytes < need))
    return fail(RBX_ERR_WORKSPACE, "capsule_bilinear_dw: workspace too small");
  float* out = splits > 1 ? static_cast<float*>(d_workspace) : d_dw;
  const int B = static_cast<int>(batch);
  switch ((dim + 31) / 32) {
    case 1: rc = cap_launch_dw<1>(d_x, x_stride_b, x_stride_l, d_g, g_stride_b, g_stride_l, d_c, B, seq_len, dim, interests, out, s); break;
    case 2: rc = cap_launch_dw<2>(d_x, x_stride_b, x_stride_l, d_g, g_stride_b, g_stride_l, d_c, B, seq_len, dim, interests, out, s); break;
    case 3: rc = cap_launch_dw<3>(d_x, x_stride_b, x_stride_l, d_g, g_stride_b, g_stride_l, d_c, B, seq_len, dim, interests, out, s); break;
    default: rc = cap_launch_dw<4>(d_x, x_stride_b, x_stride_l, d_g, g_stride_b, g_stride_l, d_c, B, seq_len, dim, interests, out, s); break;
  }
  if (rc != RBX_OK) return rc;
  if (splits > 1)
    hipLaunchKernelGGL(capsule_reduce_kernel, dim3(static_cast<unsigned>((total + 255) / 256)), dim3(256), 0, s, out, splits,
                       total, d_dw);
  return check_launch("capsule_bilinear_dw");
}
