// rbx_gru.hip -- the GRU recurrence of the session-based matching models (gfx950, wave64).  Replaces torch.nn.GRU under
// rechub's GRU4Rec (third_party/rechub/models/matching/gru4rec.py:40-44, 66-67) and NARM (narm.py:30, 50-55), including what
// NARM gets from pack_padded_sequence / pad_packed_sequence: per-sample lengths read on the device.
//
// torch's gate convention (rows of W_hh [3H, H] ordered r, z, n):
//   gh = h W_hh^T + b_hh     r = s(gi_r + gh_r)     z = s(gi_z + gh_z)     n = tanh(gi_n + r gh_n)     h' = (1 - z) n + z h
// gi = x W_ih^T + b_ih for all B L positions is one call of the dense path in front of the recurrence.
//
// gru_fwd_kernel  ONE launch walks t = 0 .. L-1.  workgroup = 16 samples, wavefront w = hidden units 16 w .. 16 w + 15 of all
//                 three gates (H / 16 rounded up wavefronts: 1 .. 8).  gh [16, 3H] = h [16, H] W_hh^T runs on
//                 v_mfma_f32_16x16x4_f32 (exact fp32; rows = samples, k = hidden unit of h, columns = the wave's units): three
//                 independent accumulator chains (r, z, n) of H / 4 instructions.  The wave's slice of W_hh is loaded ONCE into
//                 3 H / 4 B-operand registers per lane and stays there for the whole walk; h is exchanged between the waves
//                 through a double-buffered [H][16] LDS image (k-major: the A operand of k-step s is the 64 floats at 64 s,
//                 lane-contiguous and conflict-free; a lane stores its unit's 4 samples as one float4): one barrier per step.
//                 The accumulator lane that owns (unit j, samples 4 q .. 4 q + 3) holds gh_r, gh_z, gh_n of the same element in
//                 the same register slot, so the gates are fused in registers.  Saved per position for the backward (saving,
//                 not recomputing: a recomputation would repeat the whole MFMA chain): r, z, n, gh_n and h_prev, [B, L, 5, H].
//                 t >= lengths[b]: the state is frozen and out[b, t, :] = 0 (packed-sequence semantics; length 0 is legal).
// gru_bwd_kernel  ONE launch walks t = L-1 .. 0 with dh in registers, the same tiling.  Per step the owning lane forms the gate
//                 gradients, stores d_gi [B, L, 3H] and d_gh_n = d_gi_n r [B, L, H], and puts d_gh (r, z, n) of its 4 samples
//                 into a double-buffered [3][H][16] LDS image; dh_prev = dh z + d_gh W_hh is three accumulator chains
//                 (one per gate, added in a fixed order) against the wave's 3 H / 4 register-held B operands
//                 (W_hh[g H + k, unit]).  Masked steps store zeros and pass dh through unchanged (their rows of the A operand
//                 are zeros).  d_h0 = dh after t = 0.
// No atomics, every sum in a fixed order: two runs give the same bits.  No host read-back; everything on the caller's stream.
#include "rbx_internal.h"

namespace rbx {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kGruTile = 16;               // samples per workgroup = rows of the MFMA
constexpr int kGruMinH = 4, kGruMaxH = 128;
constexpr int kGruSaved = 5;               // r, z, n, gh_n, h_prev

__device__ __forceinline__ float gru_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }
__device__ __forceinline__ float gru_tanh(float x) { return 2.f / (1.f + expf(-2.f * x)) - 1.f; }

// lengths of the lane's 4 samples, clamped to [0, L]; 0 for rows beyond the batch
__device__ __forceinline__ void gru_lengths(const void* lengths, int len_dt, long long b_first, long long B, int L,
                                            int (&len)[4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const long long b = b_first + r;
    long long v = 0;
    if (b < B) v = lengths != nullptr ? load_id(lengths, b, len_dt) : L;
    len[r] = static_cast<int>(v < 0 ? 0 : (v > L ? L : v));
  }
}

// KSMAX = k-steps (of 4 hidden units) the register file is laid out for: H <= 4 KSMAX; blockDim.x = 64 ceil(H / 16)
template <int KSMAX>
__global__ __launch_bounds__(16 * KSMAX) void gru_fwd_kernel(
    const float* __restrict__ gi, const long long gs_b, const long long gs_t, const float* __restrict__ w_hh,
    const float* __restrict__ b_hh, const float* __restrict__ h0, const void* __restrict__ lengths, const int len_dt,
    const long long B, const int L, const int H, float* __restrict__ out, float* __restrict__ saved, float* __restrict__ hn) {
  __shared__ __attribute__((aligned(16))) float hs[2][KSMAX * 4 * kGruTile];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, col = lane & 15, quad = lane >> 4;
  const int j = wv * 16 + col;
  const bool jok = j < H;
  const int nks = H >> 2;
  const long long b_first = static_cast<long long>(blockIdx.x) * kGruTile + quad * 4;

  float w[3][KSMAX];                       // B operand of k-step s, gate g: W_hh[g H + j, 4 s + quad]
#pragma unroll
  for (int g = 0; g < 3; ++g)
#pragma unroll
    for (int s = 0; s < KSMAX; ++s)
      w[g][s] = (jok && s < nks) ? w_hh[(static_cast<long long>(g) * H + j) * H + 4 * s + quad] : 0.f;
  float bias[3] = {0.f, 0.f, 0.f};
  if (b_hh != nullptr && jok) {
#pragma unroll
    for (int g = 0; g < 3; ++g) bias[g] = b_hh[g * H + j];
  }
  int len[4];
  gru_lengths(lengths, len_dt, b_first, B, L, len);
  float h[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) h[r] = (h0 != nullptr && jok && b_first + r < B) ? h0[(b_first + r) * H + j] : 0.f;
  if (jok) *reinterpret_cast<float4*>(&hs[0][j * kGruTile + quad * 4]) = make_float4(h[0], h[1], h[2], h[3]);

  for (int t = 0; t < L; ++t) {
    __syncthreads();                       // the states of step t - 1 are in hs[t & 1]; its other half is free to overwrite
    const float* cur = hs[t & 1];
    float x[3][4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool act = jok && t < len[r];
      const float* p = gi + (b_first + r) * gs_b + t * gs_t + j;
#pragma unroll
      for (int g = 0; g < 3; ++g) x[g][r] = act ? p[g * H] : 0.f;
    }
    f32x4 acc[3];
#pragma unroll
    for (int g = 0; g < 3; ++g) acc[g] = f32x4{bias[g], bias[g], bias[g], bias[g]};
#pragma unroll
    for (int s = 0; s < KSMAX; ++s) {
      if (s < nks) {
        const float a = cur[64 * s + lane];          // h[sample col][unit 4 s + quad]
#pragma unroll
        for (int g = 0; g < 3; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, w[g][s], acc[g], 0, 0, 0);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float rg = gru_sigmoid(x[0][r] + acc[0][r]);
      const float zg = gru_sigmoid(x[1][r] + acc[1][r]);
      const float ng = gru_tanh(x[2][r] + rg * acc[2][r]);
      const float hnew = ng + zg * (h[r] - ng);
      const bool act = t < len[r];
      if (jok && b_first + r < B) {
        const long long pos = (b_first + r) * L + t;
        float* sv = saved + pos * (kGruSaved * H) + j;
        sv[0] = rg; sv[H] = zg; sv[2 * H] = ng; sv[3 * H] = acc[2][r]; sv[4 * H] = h[r];
        out[pos * H + j] = act ? hnew : 0.f;
      }
      if (act) h[r] = hnew;
    }
    if (jok) *reinterpret_cast<float4*>(&hs[(t + 1) & 1][j * kGruTile + quad * 4]) = make_float4(h[0], h[1], h[2], h[3]);
  }
  if (jok) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (b_first + r < B) hn[(b_first + r) * H + j] = h[r];
  }
}

template <int KSMAX>
__global__ __launch_bounds__(16 * KSMAX) void gru_bwd_kernel(
    const float* __restrict__ saved, const float* __restrict__ w_hh, const float* __restrict__ dout, const long long os_b,
    const long long os_t, const float* __restrict__ dhn, const void* __restrict__ lengths, const int len_dt, const long long B,
    const int L, const int H, float* __restrict__ dgi, float* __restrict__ dghn, float* __restrict__ dh0) {
  __shared__ __attribute__((aligned(16))) float ds[2][3][KSMAX * 4 * kGruTile];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, col = lane & 15, quad = lane >> 4;
  const int j = wv * 16 + col;
  const bool jok = j < H;
  const int nks = H >> 2;
  const long long b_first = static_cast<long long>(blockIdx.x) * kGruTile + quad * 4;

  float w[3][KSMAX];                       // B operand of k-step s, gate g: W_hh[g H + 4 s + quad, j]
#pragma unroll
  for (int g = 0; g < 3; ++g)
#pragma unroll
    for (int s = 0; s < KSMAX; ++s)
      w[g][s] = (jok && s < nks) ? w_hh[(static_cast<long long>(g) * H + 4 * s + quad) * H + j] : 0.f;
  int len[4];
  gru_lengths(lengths, len_dt, b_first, B, L, len);
  float dh[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) dh[r] = (dhn != nullptr && jok && b_first + r < B) ? dhn[(b_first + r) * H + j] : 0.f;

  for (int t = L - 1; t >= 0; --t) {
    float (*buf)[KSMAX * 4 * kGruTile] = ds[t & 1];
    float carry[4], dg[3][4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool act = jok && t < len[r];
      const long long pos = (b_first + r) * L + t;
      carry[r] = dh[r];
      dg[0][r] = dg[1][r] = dg[2][r] = 0.f;
      float dnp = 0.f;
      if (act) {
        const float* sv = saved + pos * (kGruSaved * H) + j;
        const float rg = sv[0], zg = sv[H], ng = sv[2 * H], ghn = sv[3 * H], hp = sv[4 * H];
        const float g = dh[r] + (dout != nullptr ? dout[(b_first + r) * os_b + t * os_t + j] : 0.f);
        dnp = g * (1.f - zg) * (1.f - ng * ng);
        dg[0][r] = dnp * ghn * rg * (1.f - rg);
        dg[1][r] = g * (hp - ng) * zg * (1.f - zg);
        dg[2][r] = dnp * rg;
        carry[r] = g * zg;
      }
      if (jok && b_first + r < B) {
        float* p = dgi + pos * (3 * H) + j;
        p[0] = dg[0][r]; p[H] = dg[1][r]; p[2 * H] = dnp;
        dghn[pos * H + j] = dg[2][r];
      }
    }
    if (jok) {
#pragma unroll
      for (int g = 0; g < 3; ++g)
        *reinterpret_cast<float4*>(&buf[g][j * kGruTile + quad * 4]) = make_float4(dg[g][0], dg[g][1], dg[g][2], dg[g][3]);
    }
    __syncthreads();                       // d_gh of step t is in ds[t & 1]; step t - 1 writes the other half
    f32x4 acc[3];
#pragma unroll
    for (int g = 0; g < 3; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < KSMAX; ++s) {
      if (s < nks) {
#pragma unroll
        for (int g = 0; g < 3; ++g)
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

static bool gru_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

static int gru_check(const char* what, int64_t batch, int32_t seq_len, int32_t hidden, int32_t dtype, const void* lengths,
                     int32_t lengths_dtype) {
  if (batch < 0) return fail(RBX_ERR_INVALID, "%s: batch=%lld", what, static_cast<long long>(batch));
  if (!rbx_gru_supported(hidden, seq_len))
    return fail(RBX_ERR_UNSUPPORTED, "%s: hidden=%d is not a multiple of 4 in [%d,%d], or seq_len=%d < 1", what, hidden,
                kGruMinH, kGruMaxH, seq_len);
  if (dtype != RBX_F32) return fail(RBX_ERR_UNSUPPORTED, "%s: tensor dtype code %d (float32 only)", what, dtype);
  if (lengths != nullptr && lengths_dtype != RBX_I32 && lengths_dtype != RBX_I64)
    return fail(RBX_ERR_UNSUPPORTED, "%s: lengths_dtype=%d", what, lengths_dtype);
  if ((batch + kGruTile - 1) / kGruTile > INT_MAX)
    return fail(RBX_ERR_UNSUPPORTED, "%s: batch=%lld is too large", what, static_cast<long long>(batch));
  return RBX_OK;
}

}  // namespace rbx

extern "C" int rbx_gru_supported(int32_t hidden, int32_t seq_len) {
  using namespace rbx;
  return seq_len >= 1 && hidden >= kGruMinH && hidden <= kGruMaxH && (hidden & 3) == 0;
}

extern "C" int rbx_gru_fwd(const float* d_gi, int64_t gi_stride_b, int64_t gi_stride_t, const float* d_w_hh,
                           const float* d_b_hh, const float* d_h0, const void* d_lengths, int32_t lengths_dtype,
                           int64_t batch, int32_t seq_len, int32_t hidden, int32_t dtype, float* d_out, float* d_saved,
                           float* d_hn, void* stream) {
  using namespace rbx;
  const int rc = gru_check("gru_fwd", batch, seq_len, hidden, dtype, d_lengths, lengths_dtype);
  if (rc != RBX_OK) return rc;
  if (batch == 0) return RBX_OK;
  if (!d_gi || !d_w_hh || !d_out || !d_saved || !d_hn) return fail(RBX_ERR_INVALID, "gru_fwd: NULL tensor");
  if (!gru_aligned(d_gi) || (gi_stride_b & 3) != 0 || (gi_stride_t & 3) != 0 || gi_stride_t < 3 * hidden)
    return fail(RBX_ERR_UNSUPPORTED, "gru_fwd: gi must be 16-byte aligned with strides that are multiples of 4 floats");
  const dim3 grid(static_cast<unsigned>((batch + kGruTile - 1) / kGruTile)), block(64 * ((hidden + 15) / 16));
  hipStream_t s = as_stream(stream);
#define RBX_GRU_FWD(KS)                                                                                                    \
  hipLaunchKernelGGL(gru_fwd_kernel<KS>, grid, block, 0, s, d_gi, gi_stride_b, gi_stride_t, d_w_hh, d_b_hh, d_h0, d_lengths, \
                     lengths_dtype, batch, seq_len, hidden, d_out, d_saved, d_hn)
  if (hidden <= 32) RBX_GRU_FWD(8);
  else if (hidden <= 64) RBX_GRU_FWD(16);
  else RBX_GRU_FWD(32);
#undef RBX_GRU_FWD
  return check_launch("gru_fwd");
}

extern "C" int rbx_gru_bwd(const float* d_saved, const float* d_w_hh, const float* d_dout, int64_t dout_stride_b,
                           int64_t dout_stride_t, const float* d_dhn, const void* d_lengths, int32_t lengths_dtype,
                           int64_t batch, int32_t seq_len, int32_t hidden, int32_t dtype, float* d_dgi, float* d_dghn,
                           float* d_dh0, void* stream) {
  using namespace rbx;
  const int rc = gru_check("gru_bwd", batch, seq_len, hidden, dtype, d_lengths, lengths_dtype);
  if (rc != RBX_OK) return rc;
  if (batch == 0) return RBX_OK;
  if (!d_saved || !d_w_hh || !d_dgi || !d_dghn || !d_dh0) return fail(RBX_ERR_INVALID, "gru_bwd: NULL tensor");
  if (d_dout != nullptr && (!gru_aligned(d_dout) || (dout_stride_b & 3) != 0 || (dout_stride_t & 3) != 0 || dout_stride_t < hidden))
    return fail(RBX_ERR_UNSUPPORTED, "gru_bwd: d_out must be 16-byte aligned with strides that are multiples of 4 floats");
  const dim3 grid(static_cast<unsigned>((batch + kGruTile - 1) / kGruTile)), block(64 * ((hidden + 15) / 16));
  hipStream_t s = as_stream(stream);
#define RBX_GRU_BWD(KS)                                                                                                    \
  hipLaunchKernelGGL(gru_bwd_kernel<KS>, grid, block, 0, s, d_saved, d_w_hh, d_dout, dout_stride_b, dout_stride_t, d_dhn,    \
                     d_lengths, lengths_dtype, batch, seq_len, hidden, d_dgi, d_dghn, d_dh0)
  if (hidden <= 32) RBX_GRU_BWD(8);
  else if (hidden <= 64) RBX_GRU_BWD(16);
  else RBX_GRU_BWD(32);
#undef RBX_GRU_BWD
  return check_launch("gru_bwd");
}
