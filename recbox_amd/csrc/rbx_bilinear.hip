// rbx_bilinear.hip -- FiBiNet's two blocks (gfx950, wave64): the SENET gate and the bilinear pair interaction.  Replaces, under
// third_party/rechub/basic/layers.py (SENETLayer, BiLinearInteractionLayer) and models/ranking/fibinet.py, P = F (F - 1) / 2
// nn.Linear calls on [B, 1, D] slices run twice per step, a torch.cat of 2 P pieces and a flatten.
//
//   z[b, f] = mean_d x[b, f, d]     h = relu(w1 z)     a = act(w2 h)                                        (gate)
//   out[b, p, :]     = (x[b, i] W_m(p)) * x[b, j]                 p = (i, j), i < j, itertools.combinations order
//   out[b, P + p, :] = (a[b, i] a[b, j]) * out[b, p, :]           (with a: the bilinear of v = x * a needs no GEMM of its own)
// m(p) = 0 (field_all), i (field_each), p (field_interaction); a matrix is stored [in, out] or, transposed, [out, in].
//
// gate_fwd_kernel   one wavefront per sample: float4 lanes along [F, D] form z (lane groups of D / 4 summed by shuffles), lane r
//                   forms h_r, lane f forms a_f; w1 / w2 sit in LDS.  x is read once.
// gate_bwd_kernel   a workgroup owns a contiguous run of samples; lane f carries dw2[f, :] and dw1[:, f] in registers over the
//                   run, the four wavefronts are added in wave order and one row per workgroup goes to the workspace;
//                   gate_tail_kernel adds the rows in ascending order.  dx = dz / D is written or added into an existing dx.
// bl_fwd_kernel     a workgroup stages 16 samples of x (and a) in LDS once and walks a run of consecutive pairs, a quarter per
//                   wavefront.  L = x_i W_m [16, D] runs on v_mfma_f32_16x16x4_f32 (exact fp32; rows = samples, k = input
//                   column, columns = output column); W comes through L2 and is reloaded only when m changes, L only when
//                   (i, m) changes.  Both output rows are stored from the accumulator layout: 64 contiguous bytes per sample.
// bl_dx_kernel      16 samples, all pairs.  dx and da of the tile live in LDS.  Phase i: wavefront w takes j = i + 1 + w, + 4, ..
//                   recomputes L, adds g L into row j (each row has one owner per phase) and keeps (g x_j) W^T and the da_i terms
//                   in registers; the four wavefronts are then added into row i in wave order.  g = dout1 + a_i a_j dout2.
// bl_dw_kernel      grid (sample chunk, pair group): a wavefront keeps the D x D accumulators of its consecutive pairs in MFMA
//                   accumulators across the whole chunk (dW_p += x_i^T (g x_j), k = the 16 samples of a tile) and writes them
//                   once; bl_dw_tail_kernel folds chunks and pairs onto their matrix in ascending order.
// No atomics, every sum in a fixed order: two runs give the same bits.  Nothing of size [B, P, D] besides out / dout exists.
#include "rbx_internal.h"

namespace rbx {

constexpr int kBlMinF = 2, kBlMaxF = 64;
constexpr int kBlTile = 16;                  // samples per tile = rows of the MFMA
constexpr int kBlBlock = 256;
constexpr int kBlDwBlocks = 512;             // target workgroups of bl_dw_kernel
constexpr int kGateMaxR = 32;
constexpr int kGateBlock = 256;
constexpr int kGateFwdGrid = 1024, kGateBwdGrid = 256;

static bool bl_dim_ok(int d) { return d == 4 || d == 8 || d == 16 || d == 32; }

// Not group_sum<16>: the offsets ascend here, which pairs the lanes in another order and rounds differently; the weight
// gradients keep their bits only with this order.
__device__ __forceinline__ float bl_sum16(float v) {
  v += __shfl_xor(v, 1, 64);
  v += __shfl_xor(v, 2, 64);
  v += __shfl_xor(v, 4, 64);
  v += __shfl_xor(v, 8, 64);
  return v;
}

// ---- the gate ------------------------------------------------------------------------------------------------------------
struct GateArgs {
  const float* x;        // x[b xsb + f xsf + d]
  long long xsb, xsf;
  const float* w1;       // [R, F]
  const float* w2;       // [F, R]
  float* a;              // [B, F]
  float* h;              // [B, R]
  const float* da;       // backward: [B, F]
  float* dx;             // backward: [B, F, D] contiguous
  float* ws;             // backward: [grid, 2, R, F]
  long long B;
  int F, D, R, act, accumulate;
};

// z of sample b into zs[0 .. F): all 64 lanes take part; ok = the sample exists
__device__ __forceinline__ void gate_mean(const GateArgs& g, long long b, bool ok, int lane, float* zs) {
  const int d4 = g.D >> 2, n = g.F * d4;
  const float inv = 1.f / static_cast<float>(g.D);
  for (int base = 0; base < n; base += 64) {
    const int idx = base + lane, f = idx / d4, q = idx - f * d4;
    float s = 0.f;
    if (ok && idx < n) {
      const float4 v = *reinterpret_cast<const float4*>(g.x + b * g.xsb + f * g.xsf + 4 * q);
      s = (v.x + v.y) + (v.z + v.w);
    }
    for (int o = d4 >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (idx < n && q == 0) zs[f] = s * inv;
  }
}

__global__ __launch_bounds__(kGateBlock) void gate_fwd_kernel(const GateArgs g) {
  __shared__ float w1s[kGateMaxR * kBlMaxF], w2s[kBlMaxF * kGateMaxR], zs[4][kBlMaxF], hs[4][kGateMaxR];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int F = g.F, R = g.R;
  for (int i = threadIdx.x; i < R * F; i += kGateBlock) {
    w1s[i] = g.w1[i];
    w2s[i] = g.w2[i];
  }
  const long long step = 4LL * gridDim.x;
  for (long long b0 = 4LL * blockIdx.x; b0 < g.B; b0 += step) {          // uniform over the workgroup
    const long long b = b0 + wave;
    const bool ok = b < g.B;
    gate_mean(g, b, ok, lane, zs[wave]);
    __syncthreads();
    if (lane < R) {
      float acc = 0.f;
      for (int f = 0; f < F; ++f) acc = fma_rn(w1s[lane * F + f], zs[wave][f], acc);
      acc = fmaxf(acc, 0.f);
      hs[wave][lane] = acc;
      if (ok) g.h[b * R + lane] = acc;
    }
    __syncthreads();
    if (lane < F && ok) {
      float acc = 0.f;
      for (int r = 0; r < R; ++r) acc = fma_rn(w2s[lane * R + r], hs[wave][r], acc);
      g.a[b * F + lane] = g.act == 0 ? fmaxf(acc, 0.f) : 1.f / (1.f + __expf(-acc));
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kGateBlock) void gate_bwd_kernel(const GateArgs g) {
  __shared__ float w1s[kGateMaxR * kBlMaxF], w2s[kBlMaxF * kGateMaxR], red[2 * kGateMaxR * kBlMaxF];
  __shared__ float zs[4][kBlMaxF], hs[4][kGateMaxR], p2[4][kBlMaxF], p1[4][kGateMaxR], dzs[4][kBlMaxF];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int F = g.F, R = g.R, d4 = g.D >> 2;
  const float inv = 1.f / static_cast<float>(g.D);
  for (int i = threadIdx.x; i < R * F; i += kGateBlock) {
    w1s[i] = g.w1[i];
    w2s[i] = g.w2[i];
  }
  const long long per = (g.B + gridDim.x - 1) / gridDim.x;
  const long long c0 = per * blockIdx.x, c1 = (c0 + per < g.B) ? c0 + per : g.B;
  float acc1[kGateMaxR], acc2[kGateMaxR];              // lane f: dw1[r, f] and dw2[f, r] over this wavefront's samples
#pragma unroll
  for (int r = 0; r < kGateMaxR; ++r) acc1[r] = acc2[r] = 0.f;

  for (long long b0 = c0; b0 < c1; b0 += 4) {          // uniform over the workgroup
    const long long b = b0 + wave;
    const bool ok = b < c1;
    gate_mean(g, b, ok, lane, zs[wave]);
    if (lane < R) hs[wave][lane] = ok ? g.h[b * R + lane] : 0.f;
    float dp2 = 0.f;
    if (lane < F && ok) {
      const float av = g.a[b * F + lane], dv = g.da[b * F + lane];
      dp2 = g.act == 0 ? (av > 0.f ? dv : 0.f) : dv * av * (1.f - av);
    }
    if (lane < F) p2[wave][lane] = dp2;
    __syncthreads();
    if (lane < R) {
      float dh = 0.f;
      for (int f = 0; f < F; ++f) dh = fma_rn(w2s[f * R + lane], p2[wave][f], dh);
      p1[wave][lane] = hs[wave][lane] > 0.f ? dh : 0.f;
    }
    __syncthreads();
    if (lane < F) {
      const float zf = ok ? zs[wave][lane] : 0.f;
      float dz = 0.f;
#pragma unroll
      for (int r = 0; r < kGateMaxR; ++r) {
        if (r < R) {
          const float d1 = p1[wave][r];
          dz = fma_rn(w1s[r * F + lane], d1, dz);
          acc1[r] = fma_rn(d1, zf, acc1[r]);
          acc2[r] = fma_rn(dp2, hs[wave][r], acc2[r]);
        }
      }
      dzs[wave][lane] = dz * inv;
    }
    __syncthreads();
    if (ok) {
      const int n = F * d4;
      for (int idx = lane; idx < n; idx += 64) {
        const int f = idx / d4;
        const float v = dzs[wave][f];
        float4* p = reinterpret_cast<float4*>(g.dx + (b * F) * g.D + 4LL * idx);
        float4 o = make_float4(v, v, v, v);
        if (g.accumulate) {
          const float4 old = *p;
          o = make_float4(old.x + v, old.y + v, old.z + v, old.w + v);
        }
        *p = o;
      }
    }
    __syncthreads();
  }

  for (int w = 0; w < 4; ++w) {                        // the four wavefronts in wave order
    if (wave == w && lane < F) {
#pragma unroll
      for (int r = 0; r < kGateMaxR; ++r) {
        if (r < R) {
          float* q1 = &red[r * F + lane];
          float* q2 = &red[R * F + r * F + lane];
          *q1 = w == 0 ? acc1[r] : *q1 + acc1[r];
          *q2 = w == 0 ? acc2[r] : *q2 + acc2[r];
        }
      }
    }
    __syncthreads();
  }
  float* row = g.ws + static_cast<long long>(blockIdx.x) * 2 * R * F;
  for (int i = threadIdx.x; i < 2 * R * F; i += kGateBlock) row[i] = red[i];
}

// dw1 [R, F] and dw2 [F, R] from the rows [rows, 2, R, F] of the workspace, in ascending row order
__global__ __launch_bounds__(256) void gate_tail_kernel(const float* ws, int rows, int R, int F, float* dw1, float* dw2) {
  const int i = blockIdx.x * 256 + threadIdx.x, n = R * F;
  if (i >= 2 * n) return;
  float s = 0.f;
  for (int k = 0; k < rows; ++k) s += ws[static_cast<long long>(k) * 2 * n + i];
  if (i < n) {
    dw1[i] = s;
  } else {
    const int r = (i - n) / F, f = (i - n) - r * F;
    dw2[f * R + r] = s;
  }
}

static int gate_bwd_grid(long long B) {
  const long long g = (B + 3) / 4;
  return static_cast<int>(g < kGateBwdGrid ? g : kGateBwdGrid);
}

static int gate_check(const char* what, const float* x, int64_t xsb, int64_t xsf, int64_t batch, int fields, int dim, int reduced,
                      int act, int dtype) {
  if (batch < 0) return fail(RBX_ERR_INVALID, "%s: batch=%lld", what, static_cast<long long>(batch));
  if (act != 0 && act != 1) return fail(RBX_ERR_INVALID, "%s: act=%d (0 = relu, 1 = sigmoid)", what, act);
  if (!rbx_senet_gate_supported(fields, dim, reduced, dtype))
    return fail(RBX_ERR_UNSUPPORTED, "%s: needs float32, fields=%d in [%d,%d], dim=%d in {4,8,16,32}, reduced=%d in [1,%d]", what,
                fields, kBlMinF, kBlMaxF, dim, reduced, kGateMaxR);
  if (batch == 0) return RBX_OK;
  if (!x) return fail(RBX_ERR_INVALID, "%s: x is NULL", what);
  if (!aligned16(x) || (xsb & 3) != 0 || (xsf & 3) != 0 || xsb < 0 || xsf < dim)
    return fail(RBX_ERR_UNSUPPORTED, "%s: x must be 16-byte aligned with strides that are multiples of 4 floats", what);
  return RBX_OK;
}

// ---- the pairs -----------------------------------------------------------------------------------------------------------
struct BlArgs {
  const float* x;        // x[b xsb + f xsf + d]
  long long xsb, xsf;
  const float* w;        // [M, D, D]
  const float* a;        // [B, F] or NULL
  float* out;            // forward: out[b os + row D + d]
  const float* dout;     // backward, same addressing
  long long os;
  float* dx;             // [B, F, D]
  float* da;             // [B, F] or NULL
  float* part;           // [chunks, P, D, D]
  long long B;
  int F, P, kind, transposed, ppb, tpc;    // ppb: pairs per workgroup (forward); tpc: tiles per chunk (dw)
};

__host__ __device__ inline int bl_row_stride(int fd) { return ((fd + 63) / 64) * 64 + 4; }   // == 4 mod 64: no bank conflicts

__device__ __forceinline__ void bl_decode(int p, int F, int* i, int* j) {
  int ii = 0, rem = p;
  while (rem >= F - 1 - ii) {
    rem -= F - 1 - ii;
    ++ii;
  }
  *i = ii;
  *j = ii + 1 + rem;
}

__device__ __forceinline__ int bl_matrix(int kind, int i, int p) { return kind == 0 ? 0 : (kind == 1 ? i : p); }

// the B operand of k-step s for B[k][n] = W_m[k][n] (fwd = true: L = x W) or W_m[n][k] (fwd = false: t W^T)
template <int D>
__device__ __forceinline__ void bl_load_w(const float* wm, int transposed, bool fwd, int col, int quad, float (&wf)[(D + 15) / 16][D / 4]) {
#pragma unroll
  for (int cb = 0; cb < (D + 15) / 16; ++cb) {
    const int n = col + 16 * cb;
#pragma unroll
    for (int s = 0; s < D / 4; ++s) {
      const int k = 4 * s + quad;
      const bool row_is_k = (transposed != 0) != fwd;       // [in, out] forward: W[k][n]
      wf[cb][s] = n < D ? (row_is_k ? wm[k * D + n] : wm[n * D + k]) : 0.f;
    }
  }
}

template <int D>
__global__ __launch_bounds__(kBlBlock) void bl_fwd_kernel(const BlArgs a) {
  constexpr int KS = D / 4, NCB = (D + 15) / 16;
  extern __shared__ __attribute__((aligned(16))) float bl_lds[];
  const int F = a.F, P = a.P, S = bl_row_stride(F * D), AS = F + 1;
  float* xs = bl_lds;                       // [16][S]
  float* as = bl_lds + kBlTile * S;         // [16][AS]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, quad = lane >> 4;
  const long long b0 = static_cast<long long>(blockIdx.x) * kBlTile;

  for (int idx = threadIdx.x; idx < kBlTile * F * KS; idx += kBlBlock) {
    const int s = idx / (F * KS), rem = idx - s * (F * KS), f = rem / KS, q = rem - f * KS;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (b0 + s < a.B) v = *reinterpret_cast<const float4*>(a.x + (b0 + s) * a.xsb + f * a.xsf + 4 * q);
    *reinterpret_cast<float4*>(xs + s * S + f * D + 4 * q) = v;
  }
  if (a.a != nullptr) {
    for (int idx = threadIdx.x; idx < kBlTile * F; idx += kBlBlock) {
      const int s = idx / F, f = idx - s * F;
      as[s * AS + f] = b0 + s < a.B ? a.a[(b0 + s) * F + f] : 0.f;
    }
  }
  __syncthreads();

  const int p_lo = blockIdx.y * a.ppb, p_hi = p_lo + a.ppb < P ? p_lo + a.ppb : P;
  const int per = (p_hi - p_lo + 3) / 4;
  const int w_lo = p_lo + wave * per, w_hi = w_lo + per < p_hi ? w_lo + per : p_hi;
  if (w_lo >= w_hi) return;
  int i, j;
  bl_decode(w_lo, F, &i, &j);
  int last_m = -1, last_i = -1;
  float wf[NCB][KS];
  f32x4 L[NCB];
  for (int p = w_lo; p < w_hi; ++p) {
    const int m = bl_matrix(a.kind, i, p);
    const bool new_w = m != last_m;
    if (new_w) bl_load_w<D>(a.w + static_cast<long long>(m) * D * D, a.transposed, true, col, quad, wf);
    if (new_w || i != last_i) {
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < KS; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xs[col * S + i * D + 4 * s + quad], wf[cb][s], acc, 0, 0, 0);
        L[cb] = acc;
      }
    }
    last_m = m;
    last_i = i;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int s = 4 * quad + r;
      if (b0 + s < a.B) {
        float* o = a.out + (b0 + s) * a.os;
        const float sc = a.a != nullptr ? mul_rn(as[s * AS + i], as[s * AS + j]) : 0.f;
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) {
          const int n = col + 16 * cb;
          if (n < D) {
            const float v = mul_rn(L[cb][r], xs[s * S + j * D + n]);
            o[static_cast<long long>(p) * D + n] = v;
            if (a.a != nullptr) o[static_cast<long long>(P + p) * D + n] = mul_rn(sc, v);
          }
        }
      }
    }
    if (++j == F) {
      ++i;
      j = i + 1;
    }
  }
}

template <int D>
__global__ __launch_bounds__(kBlBlock) void bl_dx_kernel(const BlArgs a) {
  constexpr int KS = D / 4, NCB = (D + 15) / 16, DP = D + 1;
  extern __shared__ __attribute__((aligned(16))) float bl_lds[];
  const int F = a.F, P = a.P, S = bl_row_stride(F * D), AS = F + 1;
  float* dxs = bl_lds;                          // [16][S]
  float* das = dxs + kBlTile * S;               // [16][AS]
  float* red = das + kBlTile * AS;              // [4][16][DP]
  float* reda = red + 4 * kBlTile * DP;         // [4][16]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, quad = lane >> 4;
  const long long b0 = static_cast<long long>(blockIdx.x) * kBlTile;
  const bool has_a = a.a != nullptr;

  for (int idx = threadIdx.x; idx < kBlTile * S; idx += kBlBlock) dxs[idx] = 0.f;
  for (int idx = threadIdx.x; idx < kBlTile * AS; idx += kBlBlock) das[idx] = 0.f;
  __syncthreads();

  const long long ba = b0 + col;                // the sample of this lane in the A-operand layout
  const bool oka = ba < a.B;
  int base = 0;                                 // index of pair (i, i + 1)
  int last_m = -1;
  float wl[NCB][KS], wt[NCB][KS];
  for (int i = 0; i + 1 < F; ++i) {
    f32x4 accI[NCB];
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) accI[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
    float daI[4] = {0.f, 0.f, 0.f, 0.f}, ai[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) ai[r] = (has_a && b0 + 4 * quad + r < a.B) ? a.a[(b0 + 4 * quad + r) * F + i] : 0.f;
    const float aia = (has_a && oka) ? a.a[ba * F + i] : 0.f;
    float xa[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) xa[s] = oka ? a.x[ba * a.xsb + i * a.xsf + 4 * s + quad] : 0.f;
    f32x4 L[NCB];
    bool have_l = false;
    for (int j = i + 1 + wave; j < F; j += 4) {
      const int p = base + (j - i - 1);
      const int m = bl_matrix(a.kind, i, p);
      if (m != last_m) {
        const float* wm = a.w + static_cast<long long>(m) * D * D;
        bl_load_w<D>(wm, a.transposed, true, col, quad, wl);
        bl_load_w<D>(wm, a.transposed, false, col, quad, wt);
        have_l = false;
      }
      last_m = m;
      if (!have_l) {
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) {
          f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int s = 0; s < KS; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[s], wl[cb][s], acc, 0, 0, 0);
          L[cb] = acc;
        }
        have_l = true;
      }
      // accumulator layout: sample 4 quad + r, column col (+ 16 cb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int s = 4 * quad + r;
        const long long b = b0 + s;
        const bool ok = b < a.B;
        const float aj = (has_a && ok) ? a.a[b * F + j] : 0.f;
        const float sc = mul_rn(ai[r], aj);
        float dsp = 0.f;
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) {
          const int n = col + 16 * cb;
          if (n < D && ok) {
            const float* dr = a.dout + b * a.os;
            const float d1 = dr[static_cast<long long>(p) * D + n];
            const float d2 = has_a ? dr[static_cast<long long>(P + p) * D + n] : 0.f;
            const float xj = a.x[b * a.xsb + j * a.xsf + n];
            const float g = fma_rn(sc, d2, d1);
            dxs[s * S + j * D + n] = fma_rn(g, L[cb][r], dxs[s * S + j * D + n]);
            dsp = fma_rn(d2, mul_rn(L[cb][r], xj), dsp);
          }
        }
        if (has_a) {
          dsp = bl_sum16(dsp);
          daI[r] = fma_rn(dsp, aj, daI[r]);
          if (col == 0) das[s * AS + j] = fma_rn(dsp, ai[r], das[s * AS + j]);
        }
      }
      // A-operand layout: sample col, column 4 s + quad: t = g x_j, dx_i += t W^T
      float t[KS];
      {
        const float sca = (has_a && oka) ? mul_rn(aia, a.a[ba * F + j]) : 0.f;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
          const int e = 4 * s + quad;
          float v = 0.f;
          if (oka) {
            const float* dr = a.dout + ba * a.os;
            const float d1 = dr[static_cast<long long>(p) * D + e];
            const float d2 = has_a ? dr[static_cast<long long>(P + p) * D + e] : 0.f;
            v = mul_rn(fma_rn(sca, d2, d1), a.x[ba * a.xsb + j * a.xsf + e]);
          }
          t[s] = v;
        }
      }
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
        for (int s = 0; s < KS; ++s) accI[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(t[s], wt[cb][s], accI[cb], 0, 0, 0);
    }
    // the four wavefronts' dx_i and da_i, added in wave order into row i
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) {
        const int n = col + 16 * cb;
        if (n < D) red[(wave * kBlTile + 4 * quad + r) * DP + n] = accI[cb][r];
      }
      if (col == 0) reda[wave * kBlTile + 4 * quad + r] = daI[r];
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < kBlTile * D; idx += kBlBlock) {
      const int s = idx / D, n = idx - s * D;
      float v = dxs[s * S + i * D + n];
      for (int w = 0; w < 4; ++w) v += red[(w * kBlTile + s) * DP + n];
      dxs[s * S + i * D + n] = v;
    }
    if (has_a && threadIdx.x < kBlTile) {
      float v = das[threadIdx.x * AS + i];
      for (int w = 0; w < 4; ++w) v += reda[w * kBlTile + threadIdx.x];
      das[threadIdx.x * AS + i] = v;
    }
    __syncthreads();
    base += F - 1 - i;
  }

  for (int idx = threadIdx.x; idx < kBlTile * F * KS; idx += kBlBlock) {
    const int s = idx / (F * KS), rem = idx - s * (F * KS);
    if (b0 + s < a.B)
      *reinterpret_cast<float4*>(a.dx + ((b0 + s) * F) * D + 4LL * rem) = *reinterpret_cast<const float4*>(dxs + s * S + 4 * rem);
  }
  if (has_a && a.da != nullptr) {
    for (int idx = threadIdx.x; idx < kBlTile * F; idx += kBlBlock) {
      const int s = idx / F, f = idx - s * F;
      if (b0 + s < a.B) a.da[(b0 + s) * F + f] = das[s * AS + f];
    }
  }
}

template <int D> struct BlDw { static constexpr int NP = D == 32 ? 4 : 8; };      // pairs a wavefront keeps accumulators for

template <int D>
__global__ __launch_bounds__(kBlBlock) void bl_dw_kernel(const BlArgs a) {
  constexpr int NCB = (D + 15) / 16, NP = BlDw<D>::NP;
  const int F = a.F, P = a.P;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 15, quad = lane >> 4;
  const bool has_a = a.a != nullptr;
  const int pw = (blockIdx.y * 4 + wave) * NP;
  if (pw >= P) return;
  int pi[NP], pj[NP];
  {
    int i, j;
    bl_decode(pw, F, &i, &j);
#pragma unroll
    for (int q = 0; q < NP; ++q) {
      pi[q] = i;
      pj[q] = j;
      if (pw + q + 1 < P && ++j == F) {
        ++i;
        j = i + 1;
      }
    }
  }
  f32x4 acc[NP][NCB][NCB];
#pragma unroll
  for (int q = 0; q < NP; ++q)
#pragma unroll
    for (int db = 0; db < NCB; ++db)
#pragma unroll
      for (int eb = 0; eb < NCB; ++eb) acc[q][db][eb] = f32x4{0.f, 0.f, 0.f, 0.f};

  const long long t0 = static_cast<long long>(blockIdx.x) * a.tpc;
  for (int tt = 0; tt < a.tpc; ++tt) {
    const long long b0 = (t0 + tt) * kBlTile;
    if (b0 >= a.B) break;
#pragma unroll
    for (int q = 0; q < NP; ++q) {
      if (pw + q < P) {
        const int p = pw + q, i = pi[q], j = pj[q];
        float xi[NCB][4], t[NCB][4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const long long b = b0 + 4 * quad + r;         // k-step r pairs lane quad with sample 4 quad + r in both operands
          const bool ok = b < a.B;
          const float sc = (has_a && ok) ? mul_rn(a.a[b * F + i], a.a[b * F + j]) : 0.f;
#pragma unroll
          for (int cb = 0; cb < NCB; ++cb) {
            const int n = col + 16 * cb;
            float xv = 0.f, tv = 0.f;
            if (ok && n < D) {
              const float* dr = a.dout + b * a.os;
              const float d1 = dr[static_cast<long long>(p) * D + n];
              const float d2 = has_a ? dr[static_cast<long long>(P + p) * D + n] : 0.f;
              tv = mul_rn(fma_rn(sc, d2, d1), a.x[b * a.xsb + j * a.xsf + n]);
              xv = a.x[b * a.xsb + i * a.xsf + n];
            }
            xi[cb][r] = xv;
            t[cb][r] = tv;
          }
        }
#pragma unroll
        for (int db = 0; db < NCB; ++db)
#pragma unroll
          for (int eb = 0; eb < NCB; ++eb)
#pragma unroll
            for (int r = 0; r < 4; ++r)
              acc[q][db][eb] = __builtin_amdgcn_mfma_f32_16x16x4f32(xi[db][r], t[eb][r], acc[q][db][eb], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int q = 0; q < NP; ++q) {
    if (pw + q < P) {
      float* o = a.part + (static_cast<long long>(blockIdx.x) * P + pw + q) * D * D;
#pragma unroll
      for (int db = 0; db < NCB; ++db)
#pragma unroll
        for (int eb = 0; eb < NCB; ++eb)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int d = 16 * db + 4 * quad + r, e = 16 * eb + col;
            if (d < D && e < D) o[d * D + e] = acc[q][db][eb][r];
          }
    }
  }
}

// dW[m] = the partials of the pairs of matrix m, pairs ascending, chunks ascending inside a pair.  One workgroup per (16
// elements, matrix): thread (el, part) adds terms part, part + 16, .. and the 16 parts are added in order.
__global__ __launch_bounds__(256) void bl_dw_tail_kernel(const float* part, int chunks, int F, int P, int D, int kind, int transposed,
                                                         float* dw) {
  __shared__ float red[16][17];
  const int el = threadIdx.x & 15, pt = threadIdx.x >> 4;
  const int m = blockIdx.y, e_idx = blockIdx.x * 16 + el;
  int pa = m, pb = m + 1;
  if (kind == 0) {
    pa = 0;
    pb = P;
  } else if (kind == 1) {
    pa = m * (F - 1) - m * (m - 1) / 2;           // pairs (m, m + 1) .. (m, F - 1); none for m = F - 1
    pb = pa + (F - 1 - m);
  }
  const long long terms = static_cast<long long>(pb - pa) * chunks, dd = static_cast<long long>(D) * D;
  float s = 0.f;
  for (long long k = pt; k < terms; k += 16) {
    const long long p = pa + k / chunks, c = k - (k / chunks) * chunks;
    s += part[(c * P + p) * dd + e_idx];
  }
  red[pt][el] = s;
  __syncthreads();
  if (pt == 0) {
    float v = red[0][el];
    for (int q = 1; q < 16; ++q) v += red[q][el];
    const int d = e_idx / D, e = e_idx - d * D;
    dw[m * dd + (transposed ? e * D + d : d * D + e)] = v;
  }
}

static int bl_pairs(int F) { return F * (F - 1) / 2; }
static int bl_matrices(int kind, int F) { return kind == 0 ? 1 : (kind == 1 ? F : bl_pairs(F)); }

static void bl_dw_split(long long B, int F, int D, int* chunks, int* tpc, int* groups) {
  const int np = D == 32 ? 4 : 8;
  const int P = bl_pairs(F);
  *groups = (P + 4 * np - 1) / (4 * np);
  const long long tiles = (B + kBlTile - 1) / kBlTile;
  long long want = kBlDwBlocks / *groups;
  if (want < 1) want = 1;
  if (want > tiles) want = tiles;
  const long long per = (tiles + want - 1) / want;
  *tpc = static_cast<int>(per);
  *chunks = static_cast<int>((tiles + per - 1) / per);
}

static size_t bl_fwd_lds(int F, int D) { return sizeof(float) * (kBlTile * bl_row_stride(F * D) + kBlTile * (F + 1)); }
static size_t bl_dx_lds(int F, int D) { return bl_fwd_lds(F, D) + sizeof(float) * (4 * kBlTile * (D + 1) + 4 * kBlTile); }

static int bl_check(const char* what, const float* x, int64_t xsb, int64_t xsf, const float* w, int64_t batch, int fields, int dim,
                    int kind, int dtype) {
  if (batch < 0) return fail(RBX_ERR_INVALID, "%s: batch=%lld", what, static_cast<long long>(batch));
  if (kind < 0 || kind > 2) return fail(RBX_ERR_INVALID, "%s: kind=%d (0 = field_all, 1 = field_each, 2 = field_interaction)", what, kind);
  if (!rbx_bilinear_pairs_supported(fields, dim, dtype))
    return fail(RBX_ERR_UNSUPPORTED, "%s: needs float32, fields=%d in [%d,%d] and dim=%d in {4,8,16,32}", what, fields, kBlMinF,
                kBlMaxF, dim);
  if (batch == 0) return RBX_OK;
  if (!x || !w) return fail(RBX_ERR_INVALID, "%s: NULL pointer", what);
  if (!aligned16(x) || (xsb & 3) != 0 || (xsf & 3) != 0 || xsb < 0 || xsf < dim)
    return fail(RBX_ERR_UNSUPPORTED, "%s: x must be 16-byte aligned with strides that are multiples of 4 floats", what);
  if ((batch + kBlTile - 1) / kBlTile > INT_MAX) return fail(RBX_ERR_UNSUPPORTED, "%s: batch=%lld is too large", what, static_cast<long long>(batch));
  return RBX_OK;
}

}  // namespace rbx

extern "C" int rbx_senet_gate_supported(int32_t fields, int32_t dim, int32_t reduced, int32_t dtype) {
  using namespace rbx;
  return dtype == RBX_F32 && fields >= kBlMinF && fields <= kBlMaxF && bl_dim_ok(dim) && reduced >= 1 && reduced <= kGateMaxR;
}

extern "C" int rbx_senet_gate_fwd(const float* d_x, int64_t x_stride_b, int64_t x_stride_f, const float* d_w1, const float* d_w2,
                                  int64_t batch, int32_t fields, int32_t dim, int32_t reduced, int32_t act, int32_t dtype,
                                  float* d_a, float* d_h, void* stream) {
  using namespace rbx;
  const int rc = gate_check("senet_gate_fwd", d_x, x_stride_b, x_stride_f, batch, fields, dim, reduced, act, dtype);
  if (rc != RBX_OK || batch == 0) return rc;
  if (!d_w1 || !d_w2 || !d_a || !d_h) return fail(RBX_ERR_INVALID, "senet_gate_fwd: NULL pointer");
  GateArgs g{};
  g.x = d_x; g.xsb = x_stride_b; g.xsf = x_stride_f; g.w1 = d_w1; g.w2 = d_w2; g.a = d_a; g.h = d_h;
  g.B = batch; g.F = fields; g.D = dim; g.R = reduced; g.act = act;
  const long long blocks = (batch + 3) / 4;
  hipLaunchKernelGGL(gate_fwd_kernel, dim3(static_cast<unsigned>(blocks < kGateFwdGrid ? blocks : kGateFwdGrid)), dim3(kGateBlock), 0,
                     as_stream(stream), g);
  return check_launch("senet_gate_fwd");
}

extern "C" size_t rbx_senet_gate_bwd_workspace_size(int64_t batch, int32_t fields, int32_t reduced) {
  using namespace rbx;
  if (batch <= 0 || fields < 1 || reduced < 1) return 0;
  return sizeof(float) * 2 * static_cast<size_t>(gate_bwd_grid(batch)) * fields * reduced;
}

extern "C" int rbx_senet_gate_bwd(const float* d_da, const float* d_x, int64_t x_stride_b, int64_t x_stride_f, const float* d_w1,
                                  const float* d_w2, const float* d_a, const float* d_h, int64_t batch, int32_t fields,
                                  int32_t dim, int32_t reduced, int32_t act, int32_t dtype, int32_t accumulate, float* d_dx,
                                  float* d_dw1, float* d_dw2, void* d_workspace, size_t workspace_bytes, void* stream) {
  using namespace rbx;
  const int rc = gate_check("senet_gate_bwd", d_x, x_stride_b, x_stride_f, batch, fields, dim, reduced, act, dtype);
  if (rc != RBX_OK || batch == 0) return rc;
  if (!d_da || !d_w1 || !d_w2 || !d_a || !d_h || !d_dx || !d_dw1 || !d_dw2 || !d_workspace)
    return fail(RBX_ERR_INVALID, "senet_gate_bwd: NULL pointer");
  if (!aligned16(d_dx)) return fail(RBX_ERR_UNSUPPORTED, "senet_gate_bwd: dx must be 16-byte aligned");
  if (workspace_bytes < rbx_senet_gate_bwd_workspace_size(batch, fields, reduced))
    return fail(RBX_ERR_WORKSPACE, "senet_gate_bwd: workspace of %zu bytes is too small", workspace_bytes);
  GateArgs g{};
  g.x = d_x; g.xsb = x_stride_b; g.xsf = x_stride_f; g.w1 = d_w1; g.w2 = d_w2;
  g.a = const_cast<float*>(d_a); g.h = const_cast<float*>(d_h); g.da = d_da; g.dx = d_dx; g.ws = static_cast<float*>(d_workspace);
  g.B = batch; g.F = fields; g.D = dim; g.R = reduced; g.act = act; g.accumulate = accumulate != 0;
  const int grid = gate_bwd_grid(batch);
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(gate_bwd_kernel, dim3(grid), dim3(kGateBlock), 0, s, g);
  int rc2 = check_launch("senet_gate_bwd");
  if (rc2 != RBX_OK) return rc2;
  hipLaunchKernelGGL(gate_tail_kernel, dim3((2 * reduced * fields + 255) / 256), dim3(256), 0, s, g.ws, grid, reduced, fields, d_dw1,
                     d_dw2);
  return check_launch("senet_gate_tail");
}

extern "C" int rbx_bilinear_pairs_supported(int32_t fields, int32_t dim, int32_t dtype) {
  using namespace rbx;
  return dtype == RBX_F32 && fields >= kBlMinF && fields <= kBlMaxF && bl_dim_ok(dim);
}

extern "C" int rbx_bilinear_pairs_fwd(const float* d_x, int64_t x_stride_b, int64_t x_stride_f, const float* d_w, const float* d_a,
                                      int64_t batch, int32_t fields, int32_t dim, int32_t kind, int32_t transposed, int32_t dtype,
                                      float* d_out, int64_t out_stride_b, void* stream) {
  using namespace rbx;
  const int rc = bl_check("bilinear_pairs_fwd", d_x, x_stride_b, x_stride_f, d_w, batch, fields, dim, kind, dtype);
  if (rc != RBX_OK || batch == 0) return rc;
  const int P = bl_pairs(fields);
  if (!d_out) return fail(RBX_ERR_INVALID, "bilinear_pairs_fwd: out is NULL");
  if (out_stride_b < static_cast<int64_t>(d_a ? 2 : 1) * P * dim)
    return fail(RBX_ERR_INVALID, "bilinear_pairs_fwd: out_stride_b=%lld is shorter than a row block", static_cast<long long>(out_stride_b));
  BlArgs a{};
  a.x = d_x; a.xsb = x_stride_b; a.xsf = x_stride_f; a.w = d_w; a.a = d_a; a.out = d_out; a.os = out_stride_b;
  a.B = batch; a.F = fields; a.P = P; a.kind = kind; a.transposed = transposed != 0;
  const long long tiles = (batch + kBlTile - 1) / kBlTile;
  long long split = (1024 + tiles - 1) / tiles;            // enough workgroups for a small batch
  if (split > 8) split = 8;
  if (split > (P + 3) / 4) split = (P + 3) / 4;
  if (split < 1) split = 1;
  a.ppb = static_cast<int>((P + split - 1) / split);
  const dim3 grid(static_cast<unsigned>(tiles), static_cast<unsigned>((P + a.ppb - 1) / a.ppb)), block(kBlBlock);
  const size_t lds = bl_fwd_lds(fields, dim);
  hipStream_t s = as_stream(stream);
  int rc_lds = RBX_OK;
#define RBX_BL_FWD(DD)                                                                      \
  if ((rc_lds = allow_lds("bilinear_pairs_fwd", bl_fwd_kernel<DD>, lds)) == RBX_OK)      \
  hipLaunchKernelGGL(bl_fwd_kernel<DD>, grid, block, lds, s, a)
  switch (dim) {
    case 4: RBX_BL_FWD(4); break;
    case 8: RBX_BL_FWD(8); break;
    case 16: RBX_BL_FWD(16); break;
    default: RBX_BL_FWD(32); break;
  }
#undef RBX_BL_FWD
  if (rc_lds != RBX_OK) return rc_lds;
  return check_launch("bilinear_pairs_fwd");
}

extern "C" size_t rbx_bilinear_pairs_bwd_workspace_size(int64_t batch, int32_t fields, int32_t dim) {
  using namespace rbx;
  if (batch <= 0 || !rbx_bilinear_pairs_supported(fields, dim, RBX_F32)) return 0;
  int chunks, tpc, groups;
  bl_dw_split(batch, fields, dim, &chunks, &tpc, &groups);
  return sizeof(float) * static_cast<size_t>(chunks) * bl_pairs(fields) * dim * dim;
}

extern "C" int rbx_bilinear_pairs_bwd(const float* d_dout, int64_t dout_stride_b, const float* d_x, int64_t x_stride_b,
                                      int64_t x_stride_f, const float* d_w, const float* d_a, int64_t batch, int32_t fields,
                                      int32_t dim, int32_t kind, int32_t transposed, int32_t dtype, float* d_dx, float* d_da,
                                      float* d_dw, void* d_workspace, size_t workspace_bytes, void* stream) {
  using namespace rbx;
  const int rc = bl_check("bilinear_pairs_bwd", d_x, x_stride_b, x_stride_f, d_w, batch, fields, dim, kind, dtype);
  if (rc != RBX_OK || batch == 0) return rc;
  const int P = bl_pairs(fields);
  if (!d_dout || !d_dx || !d_dw || !d_workspace) return fail(RBX_ERR_INVALID, "bilinear_pairs_bwd: NULL pointer");
  if (!aligned16(d_dx)) return fail(RBX_ERR_UNSUPPORTED, "bilinear_pairs_bwd: dx must be 16-byte aligned");
  if (dout_stride_b < static_cast<int64_t>(d_a ? 2 : 1) * P * dim)
    return fail(RBX_ERR_INVALID, "bilinear_pairs_bwd: dout_stride_b=%lld is shorter than a row block", static_cast<long long>(dout_stride_b));
  if (workspace_bytes < rbx_bilinear_pairs_bwd_workspace_size(batch, fields, dim))
    return fail(RBX_ERR_WORKSPACE, "bilinear_pairs_bwd: workspace of %zu bytes is too small", workspace_bytes);
  BlArgs a{};
  a.x = d_x; a.xsb = x_stride_b; a.xsf = x_stride_f; a.w = d_w; a.a = d_a; a.dout = d_dout; a.os = dout_stride_b;
  a.dx = d_dx; a.da = d_da; a.part = static_cast<float*>(d_workspace);
  a.B = batch; a.F = fields; a.P = P; a.kind = kind; a.transposed = transposed != 0;
  int chunks, groups;
  bl_dw_split(batch, fields, dim, &chunks, &a.tpc, &groups);
  const long long tiles = (batch + kBlTile - 1) / kBlTile;
  const dim3 grid_dx(static_cast<unsigned>(tiles)), grid_dw(chunks, groups), block(kBlBlock);
  const dim3 grid_tail(dim * dim / 16, bl_matrices(kind, fields));
  const size_t lds = bl_dx_lds(fields, dim);
  hipStream_t s = as_stream(stream);
  int rc_lds = RBX_OK;
#define RBX_BL_BWD(DD)                                                                          \
  if ((rc_lds = allow_lds("bilinear_pairs_bwd", bl_dx_kernel<DD>, lds)) == RBX_OK) {         \
    hipLaunchKernelGGL(bl_dx_kernel<DD>, grid_dx, block, lds, s, a);                            \
    hipLaunchKernelGGL(bl_dw_kernel<DD>, grid_dw, block, 0, s, a);                              \
  }
  switch (dim) {
    case 4: RBX_BL_BWD(4); break;
    case 8: RBX_BL_BWD(8); break;
    case 16: RBX_BL_BWD(16); break;
    default: RBX_BL_BWD(32); break;
  }
#undef RBX_BL_BWD
  if (rc_lds != RBX_OK) return rc_lds;
  const int rc2 = check_launch("bilinear_pairs_bwd");
  if (rc2 != RBX_OK) return rc2;
  hipLaunchKernelGGL(bl_dw_tail_kernel, grid_tail, dim3(256), 0, s, a.part, chunks, fields, P, dim, kind, a.transposed, d_dw);
  return check_launch("bilinear_pairs_dw_tail");
}
