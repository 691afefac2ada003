// rbx_attgru.hip -- the attention-gated GRU recurrence of DIEN's interest-evolving layer (gfx950, wave64).  Replaces RecBole's
// DynamicRNN over AGRUCell / AUGRUCell (third_party/recbole/model/sequential_recommender/dien.py:389-521: a Python loop over
// the time steps of a PackedSequence, two F.linear and a dozen element-wise launches per step, lengths copied to the host).
//
// The reference's gate convention (rows of W_hh [3H, H] ordered r, u, n: its chunk(3, 1), torch's r, z, n), a = att[b, t]:
//   gh = h W_hh^T + b_hh     r = s(gi_r + gh_r)     u = s(gi_u + gh_u)     n = tanh(gi_n + r gh_n)
//   AUGRU (cell 1): c = a u     AGRU (cell 0): c = a  (u is not formed)     h' = (1 - c) h + c n
// The blend is the other way round from torch's GRU (h' = (1 - z) n + z h), and the score has a gradient of its own.
// gi = x W_ih^T + b_ih for all B L positions is one call of the dense path in front of the recurrence.
//
// attgru_fwd_kernel  ONE launch walks t = 0 .. L-1, with gru_fwd_kernel's tiling (rbx_gru.hip): workgroup = 16 samples,
//                    wavefront w = hidden units 16 w .. 16 w + 15 of all gates, gh on v_mfma_f32_16x16x4_f32 against the wave's
//                    register-held slice of W_hh, h exchanged through a double-buffered [H][16] LDS image, one barrier per step,
//                    the gates fused in the accumulator lanes.  New: one score per sample and step (the lane's 4 samples), the
//                    blend above; AGRU runs two accumulator chains (r, n) instead of three.  Saved per position for the
//                    backward, the GRU's layout [B, L, 5, H]: r, u, n, gh_n, h_prev (AGRU leaves the u slot unwritten).
//                    t >= lengths[b]: the state is frozen and out[b, t, :] = 0 (length 0 is legal).
// attgru_bwd_kernel  ONE launch walks t = L-1 .. 0 with dh in registers, g = dout[b, t] + dh:
//                      dc = g (n - h_prev)   dn = g c   dh_prev = g (1 - c) + d_gh W_hh
//                      d_gi_n = dn (1 - n^2)   d_gh_n = d_gi_n r   d_gi_r = d_gi_n gh_n r (1 - r)
//                      AUGRU: d_gi_u = dc a u (1 - u), d_att[b, t] = sum_j dc_j u_j     AGRU: d_gi_u = 0, d_att[b, t] = sum_j dc_j
//                    d_att is summed over a wave's 16 units by a fixed cross-lane tree (lanes of units >= H add zero), then over
//                    the waves in ascending order through a double-buffered [waves][16] LDS array that rides the step's one
//                    barrier.  Masked steps store zeros into d_gi, d_gh_n and d_att and pass dh through.  d_h0 = dh after t = 0.
// No atomics, every sum in a fixed order: two runs give the same bits.  No host read-back; everything on the caller's stream.
#include "rbx_internal.h"

namespace rbx {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kAttGruTile = 16;            // samples per workgroup = rows of the MFMA
constexpr int kAttGruMinH = 4, kAttGruMaxH = 128;
constexpr int kAttGruSaved = 5;            // r, u, n, gh_n, h_prev
constexpr int kAttGruMaxWaves = kAttGruMaxH / 16;

__device__ __forceinline__ float attgru_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }
__device__ __forceinline__ float attgru_tanh(float x) { return 2.f / (1.f + expf(-2.f * x)) - 1.f; }

// lengths of the lane's 4 samples, clamped to [0, L]; 0 for rows beyond the batch
__device__ __forceinline__ void attgru_lengths(const void* lengths, int len_dt, long long b_first, long long B, int L,
                                               int (&len)[4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const long long b = b_first + r;
    long long v = 0;
    if (b < B) v = lengths != nullptr ? load_id(lengths, b, len_dt) : L;
    len[r] = static_cast<int>(v < 0 ? 0 : (v > L ? L : v));
  }
}

// KSMAX = k-steps (of 4 hidden units) the register file is laid out for: H <= 4 KSMAX; blockDim.x = 64 ceil(H / 16).
// CELL 0 = AGRU, 1 = AUGRU
template <int KSMAX, int CELL>
__global__ __launch_bounds__(16 * KSMAX) void attgru_fwd_kernel(
    const float* __restrict__ gi, const long long gs_b, const long long gs_t, const float* __restrict__ att,
    const float* __restrict__ w_hh, const float* __restrict__ b_hh, const float* __restrict__ h0,
    const void* __restrict__ lengths, const int len_dt, const long long B, const int L, const int H, float* __restrict__ out,
    float* __restrict__ saved, float* __restrict__ hn) {
  __shared__ __attribute__((aligned(16))) float hs[2][KSMAX * 4 * kAttGruTile];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, col = lane & 15, quad = lane >> 4;
  const int j = wv * 16 + col;
  const bool jok = j < H;
  const int nks = H >> 2;
  const long long b_first = static_cast<long long>(blockIdx.x) * kAttGruTile + quad * 4;

  float w[3][KSMAX];                       // B operand of k-step s, gate g: W_hh[g H + j, 4 s + quad]  (AGRU: g = 1 unused)
#pragma unroll
  for (int g = 0; g < 3; ++g)
#pragma unroll
    for (int s = 0; s < KSMAX; ++s)
      w[g][s] = ((CELL == 1 || g != 1) && jok && s < nks) ? w_hh[(static_cast<long long>(g) * H + j) * H + 4 * s + quad] : 0.f;
  float bias[3] = {0.f, 0.f, 0.f};
  if (b_hh != nullptr && jok) {
#pragma unroll
    for (int g = 0; g < 3; ++g) bias[g] = b_hh[g * H + j];
  }
  int len[4];
  attgru_lengths(lengths, len_dt, b_first, B, L, len);
  float h[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) h[r] = (h0 != nullptr && jok && b_first + r < B) ? h0[(b_first + r) * H + j] : 0.f;
  if (jok) *reinterpret_cast<float4*>(&hs[0][j * kAttGruTile + quad * 4]) = make_float4(h[0], h[1], h[2], h[3]);

  for (int t = 0; t < L; ++t) {
    __syncthreads();                       // the states of step t - 1 are in hs[t & 1]; its other half is free to overwrite
    const float* cur = hs[t & 1];
    float x[3][4], a[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool act = jok && t < len[r];  // t < len[r] implies b_first + r < B
      const float* p = gi + (b_first + r) * gs_b + t * gs_t + j;
#pragma unroll
      for (int g = 0; g < 3; ++g) x[g][r] = (act && (CELL == 1 || g != 1)) ? p[g * H] : 0.f;
      a[r] = act ? att[(b_first + r) * L + t] : 0.f;
    }
    f32x4 acc[3];
#pragma unroll
    for (int g = 0; g < 3; ++g) acc[g] = f32x4{bias[g], bias[g], bias[g], bias[g]};
#pragma unroll
    for (int s = 0; s < KSMAX; ++s) {
      if (s < nks) {
        const float av = cur[64 * s + lane];         // h[sample col][unit 4 s + quad]
#pragma unroll
        for (int g = 0; g < 3; ++g)
          if (CELL == 1 || g != 1) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, w[g][s], acc[g], 0, 0, 0);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float rg = attgru_sigmoid(x[0][r] + acc[0][r]);
      const float ug = CELL == 1 ? attgru_sigmoid(x[1][r] + acc[1][r]) : 0.f;
      const float ng = attgru_tanh(x[2][r] + rg * acc[2][r]);
      const float c = CELL == 1 ? a[r] * ug : a[r];
      const float hnew = (1.f - c) * h[r] + c * ng;
      const bool act = t < len[r];
      if (jok && b_first + r < B) {
        const long long pos = (b_first + r) * L + t;
        float* sv = saved + pos * (kAttGruSaved * H) + j;
        sv[0] = rg; sv[2 * H] = ng; sv[3 * H] = acc[2][r]; sv[4 * H] = h[r];
        if (CELL == 1) sv[H] = ug;
        out[pos * H + j] = act ? hnew : 0.f;
      }
      if (act) h[r] = hnew;
    }
    if (jok) *reinterpret_cast<float4*>(&hs[(t + 1) & 1][j * kAttGruTile + quad * 4]) = make_float4(h[0], h[1], h[2], h[3]);
  }
  if (jok) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (b_first + r < B) hn[(b_first + r) * H + j] = h[r];
  }
}

template <int KSMAX, int CELL>
__global__ __launch_bounds__(16 * KSMAX) void attgru_bwd_kernel(
    const float* __restrict__ saved, const float* __restrict__ att, const float* __restrict__ w_hh,
    const float* __restrict__ dout, const long long os_b, const long long os_t, const float* __restrict__ dhn,
    const void* __restrict__ lengths, const int len_dt, const long long B, const int L, const int H, float* __restrict__ dgi,
    float* __restrict__ dghn, float* __restrict__ datt, float* __restrict__ dh0) {
  __shared__ __attribute__((aligned(16))) float ds[2][3][KSMAX * 4 * kAttGruTile];
  __shared__ float da[2][kAttGruMaxWaves][kAttGruTile];      // per wave: the score gradient of the 16 samples over its 16 units
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, col = lane & 15, quad = lane >> 4;
  const int j = wv * 16 + col;
  const bool jok = j < H;
  const int nks = H >> 2, nwaves = blockDim.x >> 6;
  const long long b_first = static_cast<long long>(blockIdx.x) * kAttGruTile + quad * 4;

  float w[3][KSMAX];                       // B operand of k-step s, gate g: W_hh[g H + 4 s + quad, j]  (AGRU: g = 1 unused)
#pragma unroll
  for (int g = 0; g < 3; ++g)
#pragma unroll
    for (int s = 0; s < KSMAX; ++s)
      w[g][s] = ((CELL == 1 || g != 1) && jok && s < nks) ? w_hh[(static_cast<long long>(g) * H + 4 * s + quad) * H + j] : 0.f;
  int len[4];
  attgru_lengths(lengths, len_dt, b_first, B, L, len);
  float dh[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) dh[r] = (dhn != nullptr && jok && b_first + r < B) ? dhn[(b_first + r) * H + j] : 0.f;

  for (int t = L - 1; t >= 0; --t) {
    float (*buf)[KSMAX * 4 * kAttGruTile] = ds[t & 1];
    float carry[4], dg[3][4], das[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool act = jok && t < len[r];  // t < len[r] implies b_first + r < B
      const long long pos = (b_first + r) * L + t;
      carry[r] = dh[r];
      dg[0][r] = dg[1][r] = dg[2][r] = 0.f;
      das[r] = 0.f;
      float dnp = 0.f;
      if (act) {
        const float* sv = saved + pos * (kAttGruSaved * H) + j;
        const float rg = sv[0], ng = sv[2 * H], ghn = sv[3 * H], hp = sv[4 * H];
        const float ug = CELL == 1 ? sv[H] : 1.f;
        const float a = att[pos];
        const float c = CELL == 1 ? a * ug : a;
        const float g = dh[r] + (dout != nullptr ? dout[(b_first + r) * os_b + t * os_t + j] : 0.f);
        const float dc = g * (ng - hp);
        dnp = g * c * (1.f - ng * ng);
        dg[0][r] = dnp * ghn * rg * (1.f - rg);
        if (CELL == 1) dg[1][r] = dc * a * ug * (1.f - ug);
        dg[2][r] = dnp * rg;
        das[r] = CELL == 1 ? dc * ug : dc;
        carry[r] = g * (1.f - c);
      }
      if (jok && b_first + r < B) {
        float* p = dgi + pos * (3 * H) + j;
        p[0] = dg[0][r]; p[H] = dg[1][r]; p[2 * H] = dnp;
        dghn[pos * H + j] = dg[2][r];
      }
    }
    // the score gradient over the wave's 16 units: a fixed butterfly inside each group of 16 lanes
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1) {
#pragma unroll
      for (int r = 0; r < 4; ++r) das[r] += __shfl_xor(das[r], m, 16);
    }
    if (col == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r) da[t & 1][wv][quad * 4 + r] = das[r];
    }
    if (jok) {
#pragma unroll
      for (int g = 0; g < 3; ++g)
        if (CELL == 1 || g != 1)
          *reinterpret_cast<float4*>(&buf[g][j * kAttGruTile + quad * 4]) = make_float4(dg[g][0], dg[g][1], dg[g][2], dg[g][3]);
    }
    __syncthreads();                       // d_gh and the waves' score sums of step t are in half t & 1; step t - 1 writes the other
    if (threadIdx.x < kAttGruTile) {
      const long long b = static_cast<long long>(blockIdx.x) * kAttGruTile + threadIdx.x;
      float sum = da[t & 1][0][threadIdx.x];
      for (int k = 1; k < nwaves; ++k) sum += da[t & 1][k][threadIdx.x];
      if (b < B) datt[b * L + t] = sum;
    }
    f32x4 acc[3];
#pragma unroll
    for (int g = 0; g < 3; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < KSMAX; ++s) {
      if (s < nks) {
#pragma unroll
        for (int g = 0; g < 3; ++g)
          if (CELL == 1 || g != 1)
            acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(buf[g][64 * s + lane], w[g][s], acc[g], 0, 0, 0);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) dh[r] = carry[r] + ((acc[0][r] + acc[1][r]) + acc[2][r]);
  }
  if (jok) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (b_first + r < B) dh0[(b_first + r) * H + j] = dh[r];
  }
}

static bool attgru_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

static int attgru_check(const char* what, int64_t batch, int32_t seq_len, int32_t hidden, int32_t cell, int32_t dtype,
                        const void* lengths, int32_t lengths_dtype) {
  if (batch < 0) return fail(RBX_ERR_INVALID, "%s: batch=%lld", what, static_cast<long long>(batch));
  if (!rbx_attgru_supported(hidden, seq_len, cell))
    return fail(RBX_ERR_UNSUPPORTED, "%s: hidden=%d is not a multiple of 4 in [%d,%d], or seq_len=%d < 1, or cell=%d is not 0 / 1",
                what, hidden, kAttGruMinH, kAttGruMaxH, seq_len, cell);
  if (dtype != RBX_F32) return fail(RBX_ERR_UNSUPPORTED, "%s: tensor dtype code %d (float32 only)", what, dtype);
  if (lengths != nullptr && lengths_dtype != RBX_I32 && lengths_dtype != RBX_I64)
    return fail(RBX_ERR_UNSUPPORTED, "%s: lengths_dtype=%d", what, lengths_dtype);
  if ((batch + kAttGruTile - 1) / kAttGruTile > INT_MAX)
    return fail(RBX_ERR_UNSUPPORTED, "%s: batch=%lld is too large", what, static_cast<long long>(batch));
  return RBX_OK;
}

}  // namespace rbx

extern "C" int rbx_attgru_supported(int32_t hidden, int32_t seq_len, int32_t cell) {
  using namespace rbx;
  return seq_len >= 1 && hidden >= kAttGruMinH && hidden <= kAttGruMaxH && (hidden & 3) == 0 && (cell == 0 || cell == 1);
}

extern "C" int rbx_attgru_fwd(const float* d_gi, int64_t gi_stride_b, int64_t gi_stride_t, const float* d_att,
                              const float* d_w_hh, const float* d_b_hh, const float* d_h0, const void* d_lengths,
                              int32_t lengths_dtype, int64_t batch, int32_t seq_len, int32_t hidden, int32_t cell,
                              int32_t dtype, float* d_out, float* d_saved, float* d_hn, void* stream) {
  using namespace rbx;
  const int rc = attgru_check("attgru_fwd", batch, seq_len, hidden, cell, dtype, d_lengths, lengths_dtype);
  if (rc != RBX_OK) return rc;
  if (batch == 0) return RBX_OK;
  if (!d_gi || !d_att || !d_w_hh || !d_out || !d_saved || !d_hn) return fail(RBX_ERR_INVALID, "attgru_fwd: NULL tensor");
  if (!attgru_aligned(d_gi) || (gi_stride_b & 3) != 0 || (gi_stride_t & 3) != 0 || gi_stride_t < 3 * hidden)
    return fail(RBX_ERR_UNSUPPORTED, "attgru_fwd: gi must be 16-byte aligned with strides that are multiples of 4 floats");
  const dim3 grid(static_cast<unsigned>((batch + kAttGruTile - 1) / kAttGruTile)), block(64 * ((hidden + 15) / 16));
  hipStream_t s = as_stream(stream);
#define RBX_ATTGRU_FWD(KS, CELL)                                                                                            \
  hipLaunchKernelGGL((attgru_fwd_kernel<KS, CELL>), grid, block, 0, s, d_gi, gi_stride_b, gi_stride_t, d_att, d_w_hh, d_b_hh, \
                     d_h0, d_lengths, lengths_dtype, batch, seq_len, hidden, d_out, d_saved, d_hn)
#define RBX_ATTGRU_FWD_H(CELL)                                                                                              \
  do {                                                                                                                      \
    if (hidden <= 32) RBX_ATTGRU_FWD(8, CELL);                                                                              \
    else if (hidden <= 64) RBX_ATTGRU_FWD(16, CELL);                                                                        \
    else RBX_ATTGRU_FWD(32, CELL);                                                                                          \
  } while (0)
  if (cell == 1) RBX_ATTGRU_FWD_H(1);
  else RBX_ATTGRU_FWD_H(0);
#undef RBX_ATTGRU_FWD_H
#undef RBX_ATTGRU_FWD
  return check_launch("attgru_fwd");
}

extern "C" int rbx_attgru_bwd(const float* d_saved, const float* d_att, const float* d_w_hh, const float* d_dout,
                              int64_t dout_stride_b, int64_t dout_stride_t, const float* d_dhn, const void* d_lengths,
                              int32_t lengths_dtype, int64_t batch, int32_t seq_len, int32_t hidden, int32_t cell,
                              int32_t dtype, float* d_dgi, float* d_dghn, float* d_datt, float* d_dh0, void* stream) {
  using namespace rbx;
  const int rc = attgru_check("attgru_bwd", batch, seq_len, hidden, cell, dtype, d_lengths, lengths_dtype);
  if (rc != RBX_OK) return rc;
  if (batch == 0) return RBX_OK;
  if (!d_saved || !d_att || !d_w_hh || !d_dgi || !d_dghn || !d_datt || !d_dh0)
    return fail(RBX_ERR_INVALID, "attgru_bwd: NULL tensor");
  if (d_dout != nullptr && (!attgru_aligned(d_dout) || (dout_stride_b & 3) != 0 || (dout_stride_t & 3) != 0 || dout_stride_t < hidden))
    return fail(RBX_ERR_UNSUPPORTED, "attgru_bwd: d_out must be 16-byte aligned with strides that are multiples of 4 floats");
  const dim3 grid(static_cast<unsigned>((batch + kAttGruTile - 1) / kAttGruTile)), block(64 * ((hidden + 15) / 16));
  hipStream_t s = as_stream(stream);
#define RBX_ATTGRU_BWD(KS, CELL)                                                                                            \
  hipLaunchKernelGGL((attgru_bwd_kernel<KS, CELL>), grid, block, 0, s, d_saved, d_att, d_w_hh, d_dout, dout_stride_b,        \
                     dout_stride_t, d_dhn, d_lengths, lengths_dtype, batch, seq_len, hidden, d_dgi, d_dghn, d_datt, d_dh0)
#define RBX_ATTGRU_BWD_H(CELL)                                                                                              \
  do {                                                                                                                      \
    if (hidden <= 32) RBX_ATTGRU_BWD(8, CELL);                                                                              \
    else if (hidden <= 64) RBX_ATTGRU_BWD(16, CELL);                                                                        \
    else RBX_ATTGRU_BWD(32, CELL);                                                                                          \
  } while (0)
  if (cell == 1) RBX_ATTGRU_BWD_H(1);
  else RBX_ATTGRU_BWD_H(0);
#undef RBX_ATTGRU_BWD_H
#undef RBX_ATTGRU_BWD
  return check_launch("attgru_bwd");
}
