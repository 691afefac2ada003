// rbx_fieldattn.hip -- AutoInt's interacting layer: one multi-head self-attention layer over the F fields of a sample (gfx950,
// wave64), with the arithmetic of nn.MultiheadAttention(E, h) called as attn(x, x, x) without masks.  Replaces the ATen chain of
// third_party/recbole/model/context_aware_recommender/autoint.py:88-98 per layer: the transpose to [F, B, E], the in-projection
// into [F, B, 3 E], three head-major copies, the [B h, F, F] scores written, soft-maxed, dropped out, re-read (and averaged over
// the heads for a result nobody reads) and the out-projection.  Per sample, x [F, E], Win [3 E, E], bin [3 E], Wout [E, E],
// bout [E], dh = E / h:
//   q | k | v = x Win^T + bin      S_t = (q_t dh^-1/2) k_t^T      P_t = softmax over the keys (max-subtracted)
//   P~_t = keep_t * P_t * 65536 / (65536 - thr16)  (dropout only)      o = concat_t P~_t v_t
//   z = o Wout^T + bout            y = z [+ res] [then relu]
//
// Both kernels: a workgroup has 1 .. 4 wavefronts (as many as the LDS holds) and every wavefront owns ONE sample at a time, as in
// rbx_afm.hip.  The workgroup stages Win and Wout in LDS once, zero padded to the 16-row MFMA tile; a wavefront stages its
// sample's x with the field rows padded to FP = 16, 32 or 48.  Every product -- both projections, q k^T, P v and the backward's
// eight -- is fa_mm: one 16 x 16 tile of v_mfma_f32_16x16x4_f32 (exact fp32) with both operands read from LDS, either of them
// transposed by the way it is addressed.  Row strides are K + 4 floats, so the 16 rows an operand read touches fall in distinct
// banks.  q, k, v, one head's probabilities and o live in the wavefront's LDS and never reach HBM.
//
// fieldattn_fwd_kernel   writes y [B, F, E] and, when asked, the pre-dropout probabilities [B, h, F, F].
// fieldattn_bwd_kernel   recomputes q, k, v, P, the dropout mask and o with the forward's code (the same bits), takes the relu
//                        mask from the saved y and forms dz, do = dz Wout, dv = P~^T do, dP~ = do v^T, dS = P~ dP~ - P sum_j
//                        (P~ dP~), dq = dS k dh^-1/2, dk = dS^T q, dx = dqkv Win.  dWin += dqkv^T x and dWout += dz^T o stay in
//                        MFMA accumulators, dbin and dbout in two registers, across all samples of the wavefront; each
//                        wavefront writes one workspace row, fieldattn_tail_kernel adds the rows in a fixed order.
// Dropout: keep(b h + t, query, key) is drop_block / drop_keep of rbx_internal.h, one Philox call per 2 x 4 block of a head's
// plane, evaluated again in the backward; nothing is stored, and p = 0 makes no Philox call.
// No atomics, every sum in a fixed order: two runs give the same bits.  No host read-back, nothing allocated, everything on the
// caller's stream.
#include "rbx_internal.h"
#include "rbx_tile16.h"

namespace rbx {

constexpr int kFaMinF = 2, kFaMaxF = 48;
constexpr int kFaMinE = 4, kFaMaxE = 32;    // dWin [3 E, E] and dWout [E, E] are held in 16 NE^2 accumulator registers
constexpr int kFaMaxH = 8;
constexpr int kFaMaxGrid = 512;             // workgroups of a launch; x up to 4 wavefronts = rows of the workspace
constexpr size_t kFaLdsCap = 160 * 1024;    // LDS of a gfx950 compute unit

struct FaArgs {
  const float* x;        // x[b xsb + f xsf + e]
  long long xsb, xsf;
  const float* win;      // [3 E, E]
  const float* bin;      // [3 E] or NULL
  const float* wout;     // [E, E]
  const float* bout;     // [E] or NULL
  const float* res;      // res[b rsb + f rsf + e] or NULL
  long long rsb, rsf;
  float* y;              // forward: [B, F, E]
  float* attn;           // forward: [B, h, F, F] or NULL
  const float* y_in;     // backward with relu: the saved y
  const float* dy;       // backward: dy[b dsb + f dsf + e]
  long long dsb, dsf;
  float* dx;             // backward: [B, F, E] or NULL
  float* dres;           // backward: [B, F, E] or NULL
  float* part;           // backward: [rows, 4 E E + 4 E] or NULL (no weight gradient wanted)
  long long B;
  int F, E, H, relu;
  float qscale;
  DropArgs drop;
};

// (its own name for pad16 of rbx_internal.h: tests/test_gpu_autoint_forms.py holds the layout lines below to their text)
static __host__ __device__ inline int fa_pad16(int n) { return pad16(n); }
static __host__ __device__ inline int fa_row_len(int E) { return 4 * E * E + 4 * E; }                    // Win | bin | Wout | bout
static __host__ __device__ inline int fa_w_floats(int E) { return (fa_pad16(3 * E) + fa_pad16(E)) * (E + 4); }
// a wavefront's LDS: x and o [FP][E + 4], qkv [FP][3 E + 4], one head's plane [FP][FP + 4]
static __host__ __device__ inline int fa_fwd_wave_floats(int F, int E) {
  const int FP = fa_pad16(F);
  return FP * (2 * (E + 4) + (3 * E + 4) + (FP + 4));
}
// ... and in the backward dz and do [FP][E + 4], dqkv [FP][3 E + 4] and a second plane
static __host__ __device__ inline int fa_bwd_wave_floats(int F, int E) {
  const int FP = fa_pad16(F);
  return FP * (4 * (E + 4) + 2 * (3 * E + 4) + 2 * (FP + 4));
}
static int fa_waves(int E, int wave_floats) {
  for (int nw = 4; nw > 1; --nw)
    if (4 * (fa_w_floats(E) + static_cast<size_t>(nw) * wave_floats) <= kFaLdsCap) return nw;
  return 1;
}
// every wavefront takes at least two samples where the batch has them, so that staging the weights is shared by two trips
static unsigned fa_grid(int64_t batch, int nw) {
  const int64_t need = (batch + 2 * nw - 1) / (2 * nw);
  return static_cast<unsigned>(need < kFaMaxGrid ? need : kFaMaxGrid);
}

// acc += A B over one 16 x 16 tile: rows m0 .. m0 + 15 of A, columns n0 .. n0 + 15 of B, k < K (a multiple of 4).  A[m][k] lies
// at a[m lda + k] (AT: a[k lda + m]), B[k][n] at b[k ldb + n] (BT: b[n ldb + k]); rows of A from mlim and columns of B from nlim
// on count as zeros and are not read.  acc[r] is row m0 + 4 quad + r, column n0 + col.
// This is the contract of mm16 / store16 (rbx_tile16.h) with klim = K and the store's mlim = FP, in the select form.  It stays:
// with mm16 the forward and backward kernels grow by 3 to 11 % in instructions, and fused forward + backward of one layer on an
// MI355X, parent / mm16 in one session, median (min - max) ms, came out at B = 4096: 26 x 16 0.339 (0.323 - 0.387) / 0.324,
// 26 x 32 1.394 (1.393 - 1.404) / 1.411, 39 x 16 1.591 (1.589 - 1.617) / 1.612, 39 x 32 2.045 (2.043 - 2.047) / 2.049; at
// B = 65 536: 3.752 (3.742 - 3.757) / 3.475, 17.000 (16.985 - 17.065) / 17.055, 22.225 (22.195 - 22.264) / 22.298, 25.041
// (24.942 - 25.118) / 25.165.  Faster at 26 x 16, but beyond the parent's spread at 26 x 32 and at two of the large shapes.
template <bool AT, bool BT>
__device__ __forceinline__ f32x4 fa_mm(const float* a, const int lda, const int m0, const int mlim, const float* b, const int ldb,
                                       const int n0, const int nlim, const int K, f32x4 acc, const int col, const int quad) {
  const bool am = m0 + col < mlim, bn = n0 + col < nlim;
  const float* ap = AT ? a + quad * lda + m0 + col : a + (m0 + col) * lda + quad;
  const float* bp = BT ? b + (n0 + col) * ldb + quad : b + quad * ldb + n0 + col;
  const int as = AT ? 4 * lda : 4, bs = BT ? 4 : 4 * ldb;
  for (int k = 0; k < K; k += 4) {
    const float av = am ? *ap : 0.f, bv = bn ? *bp : 0.f;
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
    ap += as;
    bp += bs;
  }
  return acc;
}

__device__ __forceinline__ void fa_store(float* c, const int ldc, const int m0, const int n0, const int nlim, const f32x4 acc,
                                         const int col, const int quad) {
  if (n0 + col < nlim) {
#pragma unroll
    for (int r = 0; r < 4; ++r) c[(m0 + 4 * quad + r) * ldc + n0 + col] = acc[r];
  }
}


// Win [3 E, E] and Wout [E, E] into LDS at row stride E + 4, rows padded with zeros to the tile: the whole workgroup
__device__ __forceinline__ void fa_stage_w(const FaArgs& g, float* wl) {
  const int E = g.E, ld = E + 4, n3 = 3 * E, rows = fa_pad16(n3) + fa_pad16(E), off = fa_pad16(n3);
  for (int i = threadIdx.x; i < rows * ld; i += blockDim.x) {
    const int r = i / ld, c = i - r * ld;
    float v = 0.f;
    if (c < E) {
      if (r < n3) v = g.win[r * E + c];
      else if (r >= off && r - off < E) v = g.wout[(r - off) * E + c];
    }
    wl[i] = v;
  }
}

// rows f < F of src[b sb + f sf + ..] into dst [FP][E + 4], zeros for the other rows and for a sample that does not exist
__device__ __forceinline__ void fa_stage(const float* src, const long long sb, const long long sf, const long long b, const bool ok,
                                         const int F, const int FP, const int E, const int lane, float* dst) {
  const int e4 = E >> 2, n = FP * e4, ld = E + 4;
  for (int idx = lane; idx < n; idx += 64) {
    const int f = idx / e4, q = idx - f * e4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ok && f < F) v = *reinterpret_cast<const float4*>(src + b * sb + f * sf + 4 * q);
    *reinterpret_cast<float4*>(dst + f * ld + 4 * q) = v;
  }
}

// qkv [FP][3 E + 4] = xs Win^T + bin, the q columns times dh^-1/2.  Ends with a barrier.
__device__ __forceinline__ void fa_project(const FaArgs& g, const float* xs, const float* wl, float* qkv, const int FP, const int col,
                                           const int quad) {
  const int E = g.E, ldx = E + 4, ldq = 3 * E + 4, n3 = 3 * E;
  for (int nt = 0; 16 * nt < n3; ++nt) {
    const int n = 16 * nt + col;
    const float bias = (g.bin != nullptr && n < n3) ? g.bin[n] : 0.f, sc = n < E ? g.qscale : 1.f;
    for (int mt = 0; 16 * mt < FP; ++mt) {
      f32x4 acc = fa_mm<false, true>(xs, ldx, 16 * mt, FP, wl, ldx, 16 * nt, n3, E, f32x4{0.f, 0.f, 0.f, 0.f}, col, quad);
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[r] = mul_rn(add_rn(acc[r], bias), sc);
      fa_store(qkv, ldq, 16 * mt, 16 * nt, n3, acc, col, quad);
    }
  }
  __syncthreads();
}

// One head of one sample: S = q_t k_t^T into pb, the softmax over the keys j < F in place (rows and columns from F on: zeros),
// the probabilities to attn when asked, P~ into qb when DROP (else P~ = P and qb is not touched), o_t = P~ v_t into ob's columns
// t dh ...  Forward and backward call this: the same instructions, the same bits.  Ends with a barrier.
template <bool DROP>
__device__ __forceinline__ void fa_head(const FaArgs& g, const float* qkv, float* pb, float* qb, float* ob, const int t, const long long b,
                                        const bool ok, const int FP, const unsigned dk0, const unsigned dk1, const int lane, const int col,
                                        const int quad) {
  const int F = g.F, E = g.E, dh = E / g.H, ldx = E + 4, ldq = 3 * E + 4, ldp = FP + 4, nft = FP >> 4;
  const float* qt = qkv + t * dh;
  const float* kt = qkv + E + t * dh;
  const float* vt = qkv + 2 * E + t * dh;
  for (int mt = 0; mt < nft; ++mt)
    for (int nt = 0; nt < nft; ++nt)
      fa_store(pb, ldp, 16 * mt, 16 * nt, FP,
               fa_mm<false, true>(qt, ldq, 16 * mt, FP, kt, ldq, 16 * nt, FP, dh, f32x4{0.f, 0.f, 0.f, 0.f}, col, quad), col, quad);
  __syncthreads();
  // four rows at a time, 16 lanes to a row
  float* attn = (g.attn != nullptr && ok) ? g.attn + (b * g.H + t) * F * F : nullptr;
  for (int i = quad; i < FP; i += 4) {
    float s[3], m = -INFINITY;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int j = col + 16 * c;
      s[c] = j < F ? pb[i * ldp + j] : -INFINITY;
      m = fmaxf(m, s[c]);
    }
    m = group_max<16, kWave>(m);
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      s[c] = (col + 16 * c) < F ? expf(s[c] - m) : 0.f;
      sum += s[c];
    }
    sum = group_sum<16, kWave>(sum);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int j = col + 16 * c;
      if (j < FP) {
        const float p = i < F ? s[c] / sum : 0.f;
        pb[i * ldp + j] = p;
        if (attn != nullptr && i < F && j < F) attn[i * F + j] = p;
      }
    }
  }
  __syncthreads();
  if (DROP) {                                // one Philox call per 2 x 4 block of the plane
    const int nbj = FP >> 2, nblk = (FP >> 1) * nbj;
    const unsigned long long bh = static_cast<unsigned long long>(b) * g.H + t;
    for (int idx = lane; idx < nblk; idx += 64) {
      const int i2 = idx / nbj, j4 = idx - i2 * nbj;
      unsigned c[4];
      drop_block(static_cast<unsigned>(i2) >> 1, static_cast<unsigned>(j4), bh, i2 & 1, dk0, dk1, c);
#pragma unroll
      for (int il = 0; il < 2; ++il) {
        const int o = (2 * i2 + il) * ldp + 4 * j4;
        const float4 p = *reinterpret_cast<const float4*>(pb + o);
        float4 d;
        d.x = drop_keep(c, il, 0, g.drop.thr16) ? p.x * g.drop.scale : 0.f;
        d.y = drop_keep(c, il, 1, g.drop.thr16) ? p.y * g.drop.scale : 0.f;
        d.z = drop_keep(c, il, 2, g.drop.thr16) ? p.z * g.drop.scale : 0.f;
        d.w = drop_keep(c, il, 3, g.drop.thr16) ? p.w * g.drop.scale : 0.f;
        *reinterpret_cast<float4*>(qb + o) = d;
      }
    }
    __syncthreads();
  }
  const float* pt = DROP ? qb : pb;
  for (int mt = 0; mt < nft; ++mt)
    for (int nt = 0; 16 * nt < dh; ++nt)
      fa_store(ob + t * dh, ldx, 16 * mt, 16 * nt, dh,
               fa_mm<false, false>(pt, ldp, 16 * mt, FP, vt, ldq, 16 * nt, dh, FP, f32x4{0.f, 0.f, 0.f, 0.f}, col, quad), col, quad);
  __syncthreads();
}

extern __shared__ __attribute__((aligned(16))) float fa_smem[];

template <bool DROP>
__global__ __launch_bounds__(256) void fieldattn_fwd_kernel(const FaArgs g) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, col = lane & 15, quad = lane >> 4, nw = blockDim.x >> 6;
  const int F = g.F, E = g.E, FP = fa_pad16(F), ldx = E + 4, ldq = 3 * E + 4;
  float* wl = fa_smem;                                                 // Win [pad16(3 E)][ldx], then Wout [pad16(E)][ldx]
  const float* wol = wl + fa_pad16(3 * E) * ldx;
  float* xs = fa_smem + fa_w_floats(E) + wv * fa_fwd_wave_floats(F, E);    // [FP][ldx]
  float* ob = xs + FP * ldx;                                           // [FP][ldx]
  float* qkv = ob + FP * ldx;                                          // [FP][ldq]
  float* pb = qkv + FP * ldq;                                          // [FP][ldp]
  fa_stage_w(g, wl);
  unsigned dk0 = 0, dk1 = 0;
  if (DROP) drop_seed(g.drop, &dk0, &dk1);

  const long long step = static_cast<long long>(gridDim.x) * nw;
  for (long long b0 = static_cast<long long>(blockIdx.x) * nw; b0 < g.B; b0 += step) {      // uniform over the workgroup
    const long long b = b0 + wv;
    const bool ok = b < g.B;
    fa_stage(g.x, g.xsb, g.xsf, b, ok, F, FP, E, lane, xs);
    __syncthreads();                         // xs (and, the first time, the weights)
    fa_project(g, xs, wl, qkv, FP, col, quad);
    for (int t = 0; t < g.H; ++t) fa_head<DROP>(g, qkv, pb, pb, ob, t, b, ok, FP, dk0, dk1, lane, col, quad);
    for (int nt = 0; 16 * nt < E; ++nt) {
      const int n = 16 * nt + col;
      const float bias = (g.bout != nullptr && n < E) ? g.bout[n] : 0.f;
      for (int mt = 0; 16 * mt < FP; ++mt) {
        const f32x4 acc = fa_mm<false, true>(ob, ldx, 16 * mt, FP, wol, ldx, 16 * nt, E, E, f32x4{0.f, 0.f, 0.f, 0.f}, col, quad);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int f = 16 * mt + 4 * quad + r;
          if (ok && f < F && n < E) {
            float v = add_rn(acc[r], bias);
            if (g.res != nullptr) v = add_rn(v, g.res[b * g.rsb + f * g.rsf + n]);
            if (g.relu) v = fmaxf(v, 0.f);
            g.y[(b * F + f) * E + n] = v;
          }
        }
      }
    }
    __syncthreads();                         // xs and ob are written again for the next sample
  }
}

template <int NE, bool DROP>
__global__ __launch_bounds__(256) void fieldattn_bwd_kernel(const FaArgs g) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, col = lane & 15, quad = lane >> 4, nw = blockDim.x >> 6;
  const int F = g.F, E = g.E, FP = fa_pad16(F), dh = E / g.H, n3 = 3 * E, ldx = E + 4, ldq = 3 * E + 4, ldp = FP + 4, nft = FP >> 4;
  float* wl = fa_smem;
  const float* wol = wl + fa_pad16(3 * E) * ldx;
  float* xs = fa_smem + fa_w_floats(E) + wv * fa_bwd_wave_floats(F, E);    // [FP][ldx]
  float* ob = xs + FP * ldx;                                           // o
  float* dzb = ob + FP * ldx;                                          // dz
  float* dob = dzb + FP * ldx;                                         // do
  float* qkv = dob + FP * ldx;                                         // [FP][ldq]
  float* dqkv = qkv + FP * ldq;                                        // [FP][ldq]
  float* pb = dqkv + FP * ldq;                                         // P of the head [FP][ldp]
  float* qb = pb + FP * ldp;                                           // P~, then P~ dP~, then dS
  fa_stage_w(g, wl);
  unsigned dk0 = 0, dk1 = 0;
  if (DROP) drop_seed(g.drop, &dk0, &dk1);
  const bool want_w = g.part != nullptr;

  f32x4 dwin[3 * NE][NE], dwout[NE][NE];  // dWin[16 m + 4 quad + r][16 n + col], dWout likewise, over this wavefront's samples
  float dbin[2] = {0.f, 0.f}, dbout = 0.f;   // dbin[lane + 64 c], dbout[lane]
#pragma unroll
  for (int n = 0; n < NE; ++n) {
#pragma unroll
    for (int m = 0; m < 3 * NE; ++m) dwin[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int m = 0; m < NE; ++m) dwout[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  const long long step = static_cast<long long>(gridDim.x) * nw;
  for (long long b0 = static_cast<long long>(blockIdx.x) * nw; b0 < g.B; b0 += step) {      // uniform over the workgroup
    const long long b = b0 + wv;
    const bool ok = b < g.B;
    fa_stage(g.x, g.xsb, g.xsf, b, ok, F, FP, E, lane, xs);
    fa_stage(g.dy, g.dsb, g.dsf, b, ok, F, FP, E, lane, dzb);
    if (g.relu && ok) {                      // the entries this lane staged
      const int e4 = E >> 2;
      for (int idx = lane; idx < F * e4; idx += 64) {
        const int f = idx / e4, q = idx - f * e4;
        const float4 yv = *reinterpret_cast<const float4*>(g.y_in + (b * F + f) * E + 4 * q);
        float4 d = *reinterpret_cast<float4*>(dzb + f * ldx + 4 * q);
        d.x = yv.x > 0.f ? d.x : 0.f;
        d.y = yv.y > 0.f ? d.y : 0.f;
        d.z = yv.z > 0.f ? d.z : 0.f;
        d.w = yv.w > 0.f ? d.w : 0.f;
        *reinterpret_cast<float4*>(dzb + f * ldx + 4 * q) = d;
        if (g.dres != nullptr) *reinterpret_cast<float4*>(g.dres + (b * F + f) * E + 4 * q) = d;
      }
    } else if (g.dres != nullptr && ok) {
      const int e4 = E >> 2;
      for (int idx = lane; idx < F * e4; idx += 64) {
        const int f = idx / e4, q = idx - f * e4;
        *reinterpret_cast<float4*>(g.dres + (b * F + f) * E + 4 * q) = *reinterpret_cast<const float4*>(dzb + f * ldx + 4 * q);
      }
    }
    __syncthreads();                         // xs, dz (and, the first time, the weights)
    fa_project(g, xs, wl, qkv, FP, col, quad);
    for (int mt = 0; mt < nft; ++mt)         // do = dz Wout
      for (int nt = 0; 16 * nt < E; ++nt)
        fa_store(dob, ldx, 16 * mt, 16 * nt, E,
                 fa_mm<false, false>(dzb, ldx, 16 * mt, FP, wol, ldx, 16 * nt, E, E, f32x4{0.f, 0.f, 0.f, 0.f}, col, quad), col, quad);
    if (want_w && lane < E) {
      float s = 0.f;
      for (int f = 0; f < F; ++f) s += dzb[f * ldx + lane];
      dbout += s;
    }
    // fa_head's first barrier orders do before its readers

    for (int t = 0; t < g.H; ++t) {
      fa_head<DROP>(g, qkv, pb, qb, ob, t, b, ok, FP, dk0, dk1, lane, col, quad);
      const float* pt = DROP ? qb : pb;
      const float* qt = qkv + t * dh;
      const float* kt = qkv + E + t * dh;
      const float* vt = qkv + 2 * E + t * dh;
      const float* dot = dob + t * dh;
      for (int mt = 0; mt < nft; ++mt)       // dv_t = P~^T do_t
        for (int nt = 0; 16 * nt < dh; ++nt)
          fa_store(dqkv + 2 * E + t * dh, ldq, 16 * mt, 16 * nt, dh,
                   fa_mm<true, false>(pt, ldp, 16 * mt, FP, dot, ldx, 16 * nt, dh, FP, f32x4{0.f, 0.f, 0.f, 0.f}, col, quad), col, quad);
      __syncthreads();                       // P~ is read; qb takes P~ dP~
      for (int mt = 0; mt < nft; ++mt)       // dP~ = do_t v_t^T
        for (int nt = 0; nt < nft; ++nt) {
          const f32x4 acc = fa_mm<false, true>(dot, ldx, 16 * mt, FP, vt, ldq, 16 * nt, FP, dh, f32x4{0.f, 0.f, 0.f, 0.f}, col, quad);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int o = (16 * mt + 4 * quad + r) * ldp + 16 * nt + col;
            qb[o] = mul_rn(pt[o], acc[r]);
          }
        }
      __syncthreads();
      for (int i = quad; i < FP; i += 4) {   // dS = P~ dP~ - P sum_j (P~ dP~): 16 lanes to a row
        float tv[3], s = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const int j = col + 16 * c;
          tv[c] = j < FP ? qb[i * ldp + j] : 0.f;
          s += tv[c];
        }
        s = group_sum<16, kWave>(s);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const int j = col + 16 * c;
          if (j < FP) qb[i * ldp + j] = fma_rn(-pb[i * ldp + j], s, tv[c]);
        }
      }
      __syncthreads();                       // dS
      for (int mt = 0; mt < nft; ++mt)
        for (int nt = 0; 16 * nt < dh; ++nt) {
          f32x4 acc = fa_mm<false, false>(qb, ldp, 16 * mt, FP, kt, ldq, 16 * nt, dh, FP, f32x4{0.f, 0.f, 0.f, 0.f}, col, quad);
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[r] = mul_rn(acc[r], g.qscale);
          fa_store(dqkv + t * dh, ldq, 16 * mt, 16 * nt, dh, acc, col, quad);                         // dq_t = dS k_t dh^-1/2
          fa_store(dqkv + E + t * dh, ldq, 16 * mt, 16 * nt, dh,                                       // dk_t = dS^T q_t
                   fa_mm<true, false>(qb, ldp, 16 * mt, FP, qt, ldq, 16 * nt, dh, FP, f32x4{0.f, 0.f, 0.f, 0.f}, col, quad), col, quad);
        }
      __syncthreads();                       // pb and qb are written again by the next head
    }

    if (g.dx != nullptr) {                   // dx = dqkv Win
      for (int mt = 0; mt < nft; ++mt)
        for (int nt = 0; 16 * nt < E; ++nt) {
          const f32x4 acc = fa_mm<false, false>(dqkv, ldq, 16 * mt, FP, wl, ldx, 16 * nt, E, n3, f32x4{0.f, 0.f, 0.f, 0.f}, col, quad);
          const int n = 16 * nt + col;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int f = 16 * mt + 4 * quad + r;
            if (ok && f < F && n < E) g.dx[(b * F + f) * E + n] = acc[r];
          }
        }
    }
    if (want_w) {                            // rows of dz, dqkv, o and x from F on are zeros
#pragma unroll
      for (int n = 0; n < NE; ++n) {
        if (16 * n < E) {
#pragma unroll
          for (int m = 0; m < 3 * NE; ++m)
            if (16 * m < n3) dwin[m][n] = fa_mm<true, false>(dqkv, ldq, 16 * m, n3, xs, ldx, 16 * n, E, FP, dwin[m][n], col, quad);
#pragma unroll
          for (int m = 0; m < NE; ++m)
            if (16 * m < E) dwout[m][n] = fa_mm<true, false>(dzb, ldx, 16 * m, E, ob, ldx, 16 * n, E, FP, dwout[m][n], col, quad);
        }
      }
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const int n = lane + 64 * c;
        if (n < n3) {
          float s = 0.f;
          for (int f = 0; f < F; ++f) s += dqkv[f * ldq + n];
          dbin[c] += s;
        }
      }
    }
    __syncthreads();                         // every buffer is written again for the next sample
  }

  if (want_w) {
    float* row = g.part + (static_cast<long long>(blockIdx.x) * nw + wv) * fa_row_len(E);
    float* rwo = row + n3 * E + n3;
#pragma unroll
    for (int n = 0; n < NE; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int c = 16 * n + col;
#pragma unroll
        for (int m = 0; m < 3 * NE; ++m) {
          const int u = 16 * m + 4 * quad + r;
          if (u < n3 && c < E) row[u * E + c] = dwin[m][n][r];
        }
#pragma unroll
        for (int m = 0; m < NE; ++m) {
          const int u = 16 * m + 4 * quad + r;
          if (u < E && c < E) rwo[u * E + c] = dwout[m][n][r];
        }
      }
#pragma unroll
    for (int c = 0; c < 2; ++c)
      if (lane + 64 * c < n3) row[n3 * E + lane + 64 * c] = dbin[c];
    if (lane < E) rwo[E * E + lane] = dbout;
  }
}

// out[e] = sum over the rows of the workspace, e < rl, in colsum16's order.  A row is Win | bin | Wout | bout; a NULL
// destination is skipped.
__global__ __launch_bounds__(256) void fieldattn_tail_kernel(const float* __restrict__ part, const int rows, const int E,
                                                             float* __restrict__ dwin, float* __restrict__ dbin,
                                                             float* __restrict__ dwout, float* __restrict__ dbout) {
  __shared__ float sm[16][17];
  const int rl = fa_row_len(E), c = threadIdx.x & 15, r = threadIdx.x >> 4, e = blockIdx.x * 16 + c;
  colsum16(part, rows, rl, e, r, c, sm);
  if (r == 0 && e < rl) {
    const int o1 = 3 * E * E, o2 = o1 + 3 * E, o3 = o2 + E * E;
    float* dst = e < o1 ? dwin : (e < o2 ? dbin : (e < o3 ? dwout : dbout));
    const int at = e < o1 ? e : (e < o2 ? e - o1 : (e < o3 ? e - o2 : e - o3));
    if (dst != nullptr) dst[at] = sm[0][c];
  }
}

static int fa_strided(const char* what, const char* name, const void* p, int64_t sb, int64_t sf, int32_t dim) {
  if (p != nullptr && (!aligned16(p) || (sb & 3) != 0 || (sf & 3) != 0 || sf < dim || sb < 0))
    return fail(RBX_ERR_UNSUPPORTED, "%s: %s must be 16-byte aligned with strides that are multiples of 4 floats", what, name);
  return RBX_OK;
}

static int fa_check(const char* what, int64_t batch, int32_t n_fields, int32_t dim, int32_t heads, int32_t dtype) {
  if (batch < 0) return fail(RBX_ERR_INVALID, "%s: batch=%lld", what, static_cast<long long>(batch));
  if (!rbx_fieldattn_supported(n_fields, dim, heads))
    return fail(RBX_ERR_UNSUPPORTED, "%s: n_fields=%d in [%d,%d], dim=%d a multiple of 4 in [%d,%d], heads=%d in [1,%d] with "
                "dim / heads a multiple of 4", what, n_fields, kFaMinF, kFaMaxF, dim, kFaMinE, kFaMaxE, heads, kFaMaxH);
  if (dtype != RBX_F32) return fail(RBX_ERR_UNSUPPORTED, "%s: tensor dtype code %d (float32 only)", what, dtype);
  return RBX_OK;
}

// the arguments of rbx_attn_dropout_fwd
static int fa_drop(const char* what, float p, uint64_t seed, const uint64_t* d_seed_add, DropArgs* d) {
  if (!(p >= 0.f) || p >= 1.f) return fail(RBX_ERR_INVALID, "%s: dropout probability %g not in [0, 1)", what, static_cast<double>(p));
  unsigned thr = static_cast<unsigned>(p * 65536.0f + 0.5f);
  if (thr > 65535u) thr = 65535u;
  d->thr16 = thr;
  d->scale = 65536.0f / static_cast<float>(65536u - thr);
  d->k0 = static_cast<unsigned>(seed);
  d->k1 = static_cast<unsigned>(seed >> 32);
  d->seed_add = reinterpret_cast<const unsigned long long*>(d_seed_add);
  return RBX_OK;
}

template <typename K>
static void fa_launch(K kernel, unsigned grid, int nw, size_t lds, hipStream_t s, const FaArgs& args) {
  // not yet allow_lds of rbx_internal.h: tests/test_gpu_autoint_forms.py holds this line and the dispatch on dim to their text
  if (lds > 64 * 1024) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(64 * nw), lds, s, args);
}

}  // namespace rbx

extern "C" int rbx_fieldattn_supported(int32_t n_fields, int32_t dim, int32_t heads) {
  using namespace rbx;
  return n_fields >= kFaMinF && n_fields <= kFaMaxF && dim >= kFaMinE && dim <= kFaMaxE && (dim & 3) == 0 && heads >= 1 &&
         heads <= kFaMaxH && dim % heads == 0 && ((dim / heads) & 3) == 0;
}

extern "C" int rbx_fieldattn_fwd(const float* d_x, int64_t x_stride_b, int64_t x_stride_f, const float* d_in_w, const float* d_in_b,
                                 const float* d_out_w, const float* d_out_b, const float* d_res, int64_t res_stride_b,
                                 int64_t res_stride_f, int32_t relu, int64_t batch, int32_t n_fields, int32_t dim, int32_t heads,
                                 int32_t dtype, float p_drop, uint64_t seed, const uint64_t* d_seed_add, float* d_y, float* d_attn,
                                 void* stream) {
  using namespace rbx;
  int rc = fa_check("fieldattn_fwd", batch, n_fields, dim, heads, dtype);
  if (rc == RBX_OK) rc = fa_strided("fieldattn_fwd", "x", d_x, x_stride_b, x_stride_f, dim);
  if (rc == RBX_OK) rc = fa_strided("fieldattn_fwd", "res", d_res, res_stride_b, res_stride_f, dim);
  FaArgs args = {};
  if (rc == RBX_OK) rc = fa_drop("fieldattn_fwd", p_drop, seed, d_seed_add, &args.drop);
  if (rc != RBX_OK) return rc;
  if (batch == 0) return RBX_OK;
  if (!d_x || !d_in_w || !d_out_w || !d_y) return fail(RBX_ERR_INVALID, "fieldattn_fwd: NULL tensor");
  args.x = d_x; args.xsb = x_stride_b; args.xsf = x_stride_f;
  args.win = d_in_w; args.bin = d_in_b; args.wout = d_out_w; args.bout = d_out_b;
  args.res = d_res; args.rsb = res_stride_b; args.rsf = res_stride_f;
  args.y = d_y; args.attn = d_attn;
  args.B = batch; args.F = n_fields; args.E = dim; args.H = heads; args.relu = relu != 0;
  args.qscale = 1.0f / sqrtf(static_cast<float>(dim / heads));
  const int wave = fa_fwd_wave_floats(n_fields, dim), nw = fa_waves(dim, wave);
  const size_t lds = 4 * (fa_w_floats(dim) + static_cast<size_t>(nw) * wave);
  if (lds > kFaLdsCap) return fail(RBX_ERR_UNSUPPORTED, "fieldattn_fwd: %zu bytes of LDS", lds);
  hipStream_t s = as_stream(stream);
  if (args.drop.thr16 != 0) fa_launch(fieldattn_fwd_kernel<true>, fa_grid(batch, nw), nw, lds, s, args);
  else fa_launch(fieldattn_fwd_kernel<false>, fa_grid(batch, nw), nw, lds, s, args);
  return check_launch("fieldattn_fwd");
}

extern "C" size_t rbx_fieldattn_bwd_workspace_size(int64_t batch, int32_t n_fields, int32_t dim, int32_t heads) {
  using namespace rbx;
  if (batch <= 0 || !rbx_fieldattn_supported(n_fields, dim, heads)) return 0;
  const int nw = fa_waves(dim, fa_bwd_wave_floats(n_fields, dim));
  return static_cast<size_t>(fa_grid(batch, nw)) * nw * fa_row_len(dim) * sizeof(float);
}

extern "C" int rbx_fieldattn_bwd(const float* d_dy, int64_t dy_stride_b, int64_t dy_stride_f, const float* d_x, int64_t x_stride_b,
                                 int64_t x_stride_f, const float* d_in_w, const float* d_in_b, const float* d_out_w, const float* d_y,
                                 int32_t relu, int64_t batch, int32_t n_fields, int32_t dim, int32_t heads, int32_t dtype,
                                 float p_drop, uint64_t seed, const uint64_t* d_seed_add, float* d_dx, float* d_dres,
                                 float* d_din_w, float* d_din_b, float* d_dout_w, float* d_dout_b, void* d_workspace,
                                 size_t workspace_bytes, void* stream) {
  using namespace rbx;
  int rc = fa_check("fieldattn_bwd", batch, n_fields, dim, heads, dtype);
  if (rc == RBX_OK) rc = fa_strided("fieldattn_bwd", "x", d_x, x_stride_b, x_stride_f, dim);
  if (rc == RBX_OK) rc = fa_strided("fieldattn_bwd", "dy", d_dy, dy_stride_b, dy_stride_f, dim);
  FaArgs args = {};
  if (rc == RBX_OK) rc = fa_drop("fieldattn_bwd", p_drop, seed, d_seed_add, &args.drop);
  if (rc != RBX_OK) return rc;
  if (batch == 0) return RBX_OK;
  if (!d_dy || !d_x || !d_in_w || !d_out_w || (relu && !d_y)) return fail(RBX_ERR_INVALID, "fieldattn_bwd: NULL tensor");
  const bool want_w = d_din_w || d_din_b || d_dout_w || d_dout_b;
  if (want_w && (d_workspace == nullptr || workspace_bytes < rbx_fieldattn_bwd_workspace_size(batch, n_fields, dim, heads)))
    return fail(RBX_ERR_WORKSPACE, "fieldattn_bwd: workspace too small");
  args.x = d_x; args.xsb = x_stride_b; args.xsf = x_stride_f;
  args.win = d_in_w; args.bin = d_in_b; args.wout = d_out_w;
  args.y_in = d_y; args.dy = d_dy; args.dsb = dy_stride_b; args.dsf = dy_stride_f;
  args.dx = d_dx; args.dres = d_dres; args.part = want_w ? static_cast<float*>(d_workspace) : nullptr;
  args.B = batch; args.F = n_fields; args.E = dim; args.H = heads; args.relu = relu != 0;
  args.qscale = 1.0f / sqrtf(static_cast<float>(dim / heads));
  const int wave = fa_bwd_wave_floats(n_fields, dim), nw = fa_waves(dim, wave);
  const size_t lds = 4 * (fa_w_floats(dim) + static_cast<size_t>(nw) * wave);
  if (lds > kFaLdsCap) return fail(RBX_ERR_UNSUPPORTED, "fieldattn_bwd: %zu bytes of LDS", lds);
  const unsigned grid = fa_grid(batch, nw);
  hipStream_t s = as_stream(stream);
  const bool drop = args.drop.thr16 != 0;
  if (dim <= 16) {
    if (drop) fa_launch(fieldattn_bwd_kernel<1, true>, grid, nw, lds, s, args);
    else fa_launch(fieldattn_bwd_kernel<1, false>, grid, nw, lds, s, args);
  } else {
    if (drop) fa_launch(fieldattn_bwd_kernel<2, true>, grid, nw, lds, s, args);
    else fa_launch(fieldattn_bwd_kernel<2, false>, grid, nw, lds, s, args);
  }
  if (want_w)
    hipLaunchKernelGGL(fieldattn_tail_kernel, dim3((fa_row_len(dim) + 15) / 16), dim3(256), 0, s, args.part,
                       static_cast<int>(grid) * nw, dim, d_din_w, d_din_b, d_dout_w, d_dout_b);
  return check_launch("fieldattn_bwd");
}
