// rbx_gru.hip -- the GRU recurrences (gfx950, wave64): ONE kernel body per direction for three cells.
//   GRU    torch.nn.GRU under rechub's GRU4Rec (third_party/rechub/models/matching/gru4rec.py:40-44, 66-67) and NARM
//          (narm.py:30, 50-55), including what NARM gets from pack_padded_sequence / pad_packed_sequence: per-sample lengths read
//          on the device.
//   AGRU / AUGRU   the attention-gated cells of DIEN's interest-evolving layer: RecBole's DynamicRNN over AGRUCell / AUGRUCell
//          (third_party/recbole/model/sequential_recommender/dien.py:389-521: a Python loop over the time steps of a
//          PackedSequence, two F.linear and a dozen element-wise launches per step, lengths copied to the host).
//
// Common to the cells (rows of W_hh [3H, H] ordered r, z, n; the reference's attention cells call z "u": its chunk(3, 1)):
//   gh = h W_hh^T + b_hh     r = s(gi_r + gh_r)     z = s(gi_z + gh_z)     n = tanh(gi_n + r gh_n)
// gi = x W_ih^T + b_ih for all B L positions is one call of the dense path in front of the recurrence.  The cells differ in the
// blend, and the attention cells read one score a = att[b, t] per sample and step, which has a gradient of its own:
//   GRU     h' = (1 - z) n + z h, computed as n + z (h - n)
//   AUGRU   c = a z     h' = (1 - c) h + c n                (cell code 1 of the C ABI)
//   AGRU    c = a       h' = (1 - c) h + c n                (cell code 0; z is not formed: two accumulator chains, r and n)
// The attention blend is the other way round from torch's GRU; each cell keeps its own expression (they round differently).
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
//                 not recomputing: a recomputation would repeat the whole MFMA chain): r, z, n, gh_n and h_prev, [B, L, 5, H]
//                 (AGRU leaves the z slot unwritten).
//                 t >= lengths[b]: the state is frozen and out[b, t, :] = 0 (packed-sequence semantics; length 0 is legal).
// gru_bwd_kernel  ONE launch walks t = L-1 .. 0 with dh in registers, the same tiling, g = dout[b, t] + dh:
//                   GRU:             dn = g (1 - z)   d_gi_z = g (h_prev - n) z (1 - z)   dh_prev = g z + d_gh W_hh
//                   AGRU / AUGRU:    dn = g c         dc = g (n - h_prev)                 dh_prev = g (1 - c) + d_gh W_hh
//                     AUGRU: d_gi_z = dc a z (1 - z), d_att[b, t] = sum_j dc_j z_j     AGRU: d_gi_z = 0, d_att[b, t] = sum_j dc_j
//                   all:             d_gi_n = dn (1 - n^2)   d_gh_n = d_gi_n r   d_gi_r = d_gi_n gh_n r (1 - r)
//                 Per step the owning lane forms the gate gradients, stores d_gi [B, L, 3H] and d_gh_n [B, L, H], and puts d_gh
//                 (r, z, n) of its 4 samples into a double-buffered [3][H][16] LDS image; d_gh W_hh is three accumulator chains
//                 (one per gate, added in a fixed order; AGRU: two) against the wave's 3 H / 4 register-held B operands
//                 (W_hh[g H + k, unit]).  d_att is summed over a wave's 16 units by a fixed cross-lane tree (lanes of units >= H
//                 add zero), then over the waves in ascending order through a double-buffered [waves][16] LDS array that rides
//                 the step's one barrier.  Masked steps store zeros into d_gi, d_gh_n and d_att and pass dh through unchanged
//                 (their rows of the A operand are zeros).  d_h0 = dh after t = 0.
// What a cell does not use (the score, the z chain, d_att and its LDS array) is compiled out of its instantiation.
// No atomics, every sum in a fixed order: two runs give the same bits.  No host read-back; everything on the caller's stream.
#include <type_traits>

#include "rbx_internal.h"

namespace rbx {

enum GruCell : int { kAgru = 0, kAugru = 1, kGru = 2 };    // the first two are the C ABI's cell codes of rbx_attgru_*

constexpr int kGruTile = 16;               // samples per workgroup = rows of the MFMA
constexpr int kGruMinH = 4, kGruMaxH = 128;
constexpr int kGruSaved = 5;               // r, z, n, gh_n, h_prev
constexpr int kGruMaxWaves = kGruMaxH / 16;

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

// KSMAX = k-steps (of 4 hidden units) the register file is laid out for: H <= 4 KSMAX; blockDim.x = 64 ceil(H / 16).
// att is read by the attention cells alone (the plain GRU is launched with NULL)
template <int KSMAX, int CELL>
__global__ __launch_bounds__(16 * KSMAX) void gru_fwd_kernel(
    const float* __restrict__ gi, const long long gs_b, const long long gs_t, const float* __restrict__ att,
    const float* __restrict__ w_hh, const float* __restrict__ b_hh, const float* __restrict__ h0,
    const void* __restrict__ lengths, const int len_dt, const long long B, const int L, const int H, float* __restrict__ out,
    float* __restrict__ saved, float* __restrict__ hn) {
  constexpr bool kAtt = CELL != kGru;      // a score per sample and step, blended the attention cells' way
  constexpr bool kZ = CELL != kAgru;       // the z gate (and its accumulator chain) exists
  __shared__ __attribute__((aligned(16))) float hs[2][KSMAX * 4 * kGruTile];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, col = lane & 15, quad = lane >> 4;
  const int j = wv * 16 + col;
  const bool jok = j < H;
  const int nks = H >> 2;
  const long long b_first = static_cast<long long>(blockIdx.x) * kGruTile + quad * 4;

  float w[3][KSMAX];                       // B operand of k-step s, gate g: W_hh[g H + j, 4 s + quad]  (AGRU: g = 1 unused)
#pragma unroll
  for (int g = 0; g < 3; ++g)
#pragma unroll
    for (int s = 0; s < KSMAX; ++s)
      w[g][s] = ((kZ || g != 1) && jok && s < nks) ? w_hh[(static_cast<long long>(g) * H + j) * H + 4 * s + quad] : 0.f;
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
    float x[3][4], a[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool act = jok && t < len[r];  // t < len[r] implies b_first + r < B
      const float* p = gi + (b_first + r) * gs_b + t * gs_t + j;
#pragma unroll
      for (int g = 0; g < 3; ++g) x[g][r] = (act && (kZ || g != 1)) ? p[g * H] : 0.f;
      if constexpr (kAtt) a[r] = act ? att[(b_first + r) * L + t] : 0.f;
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
          if (kZ || g != 1) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, w[g][s], acc[g], 0, 0, 0);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float rg = sigmoidf_fast(x[0][r] + acc[0][r]);
      const float zg = kZ ? sigmoidf_fast(x[1][r] + acc[1][r]) : 0.f;
      const float ng = tanhf_fast(x[2][r] + rg * acc[2][r]);
      float hnew;
      if constexpr (kAtt) {
        const float c = kZ ? a[r] * zg : a[r];
        hnew = (1.f - c) * h[r] + c * ng;
      } else {
        hnew = ng + zg * (h[r] - ng);
      }
      const bool act = t < len[r];
      if (jok && b_first + r < B) {
        const long long pos = (b_first + r) * L + t;
        float* sv = saved + pos * (kGruSaved * H) + j;
        sv[0] = rg; sv[2 * H] = ng; sv[3 * H] = acc[2][r]; sv[4 * H] = h[r];
        if constexpr (kZ) sv[H] = zg;
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

// att and datt belong to the attention cells alone (the plain GRU is launched with NULL for both)
template <int KSMAX, int CELL>
__global__ __launch_bounds__(16 * KSMAX) void gru_bwd_kernel(
    const float* __restrict__ saved, const float* __restrict__ att, const float* __restrict__ w_hh,
    const float* __restrict__ dout, const long long os_b, const long long os_t, const float* __restrict__ dhn,
    const void* __restrict__ lengths, const int len_dt, const long long B, const int L, const int H, float* __restrict__ dgi,
    float* __restrict__ dghn, float* __restrict__ datt, float* __restrict__ dh0) {
  constexpr bool kAtt = CELL != kGru, kZ = CELL != kAgru;
  __shared__ __attribute__((aligned(16))) float ds[2][3][KSMAX * 4 * kGruTile];
  // per wave: the score gradient of the 16 samples over its 16 units (the plain GRU never touches it, so it owns no LDS for it)
  __shared__ float da[2][kAtt ? kGruMaxWaves : 1][kGruTile];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, col = lane & 15, quad = lane >> 4;
  const int j = wv * 16 + col;
  const bool jok = j < H;
  const int nks = H >> 2, nwaves = blockDim.x >> 6;
  const long long b_first = static_cast<long long>(blockIdx.x) * kGruTile + quad * 4;

  float w[3][KSMAX];                       // B operand of k-step s, gate g: W_hh[g H + 4 s + quad, j]  (AGRU: g = 1 unused)
#pragma unroll
  for (int g = 0; g < 3; ++g)
#pragma unroll
    for (int s = 0; s < KSMAX; ++s)
      w[g][s] = ((kZ || g != 1) && jok && s < nks) ? w_hh[(static_cast<long long>(g) * H + 4 * s + quad) * H + j] : 0.f;
  int len[4];
  gru_lengths(lengths, len_dt, b_first, B, L, len);
  float dh[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) dh[r] = (dhn != nullptr && jok && b_first + r < B) ? dhn[(b_first + r) * H + j] : 0.f;

  for (int t = L - 1; t >= 0; --t) {
    float (*buf)[KSMAX * 4 * kGruTile] = ds[t & 1];
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
        const float* sv = saved + pos * (kGruSaved * H) + j;   // (the order of these loads moves the VGPR count by up to 4)
        const float rg = sv[0], zg = kZ ? sv[H] : 1.f, ng = sv[2 * H], ghn = sv[3 * H], hp = sv[4 * H];
        const float a = kAtt ? att[pos] : 0.f;       // a, c, dc: the attention cells' alone
        const float c = kZ ? a * zg : a;
        const float g = dh[r] + (dout != nullptr ? dout[(b_first + r) * os_b + t * os_t + j] : 0.f);
        const float dc = g * (ng - hp);
        dnp = kAtt ? g * c * (1.f - ng * ng) : g * (1.f - zg) * (1.f - ng * ng);
        dg[0][r] = dnp * ghn * rg * (1.f - rg);
        if (kZ) dg[1][r] = kAtt ? dc * a * zg * (1.f - zg) : g * (hp - ng) * zg * (1.f - zg);
        dg[2][r] = dnp * rg;
        das[r] = kZ ? dc * zg : dc;
        carry[r] = kAtt ? g * (1.f - c) : g * zg;
      }
      if (jok && b_first + r < B) {
        float* p = dgi + pos * (3 * H) + j;
        p[0] = dg[0][r]; p[H] = dg[1][r]; p[2 * H] = dnp;
        dghn[pos * H + j] = dg[2][r];
      }
    }
    if constexpr (kAtt) {
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
    }
    if (jok) {
#pragma unroll
      for (int g = 0; g < 3; ++g)
        if (kZ || g != 1)
          *reinterpret_cast<float4*>(&buf[g][j * kGruTile + quad * 4]) = make_float4(dg[g][0], dg[g][1], dg[g][2], dg[g][3]);
    }
    __syncthreads();                       // d_gh and the waves' score sums of step t are in half t & 1; step t - 1 writes the other
    if constexpr (kAtt) {
      if (threadIdx.x < kGruTile) {
        const long long b = static_cast<long long>(blockIdx.x) * kGruTile + threadIdx.x;
        float sum = da[t & 1][0][threadIdx.x];
        for (int k = 1; k < nwaves; ++k) sum += da[t & 1][k][threadIdx.x];
        if (b < B) datt[b * L + t] = sum;
      }
    }
    f32x4 acc[3];
#pragma unroll
    for (int g = 0; g < 3; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < KSMAX; ++s) {
      if (s < nks) {
#pragma unroll
        for (int g = 0; g < 3; ++g)
          if (kZ || g != 1) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(buf[g][64 * s + lane], w[g][s], acc[g], 0, 0, 0);
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

// cell: NULL for the plain GRU's entry points, else the C ABI's cell code (0 / 1) as the caller gave it
static int gru_check(const char* what, int64_t batch, int32_t seq_len, int32_t hidden, const int32_t* cell, int32_t dtype,
                     const void* lengths, int32_t lengths_dtype) {
  if (batch < 0) return fail(RBX_ERR_INVALID, "%s: batch=%lld", what, static_cast<long long>(batch));
  if (cell == nullptr && !rbx_gru_supported(hidden, seq_len))
    return fail(RBX_ERR_UNSUPPORTED, "%s: hidden=%d is not a multiple of 4 in [%d,%d], or seq_len=%d < 1", what, hidden,
                kGruMinH, kGruMaxH, seq_len);
  if (cell != nullptr && !rbx_attgru_supported(hidden, seq_len, *cell))
    return fail(RBX_ERR_UNSUPPORTED, "%s: hidden=%d is not a multiple of 4 in [%d,%d], or seq_len=%d < 1, or cell=%d is not 0 / 1",
                what, hidden, kGruMinH, kGruMaxH, seq_len, *cell);
  if (dtype != RBX_F32) return fail(RBX_ERR_UNSUPPORTED, "%s: tensor dtype code %d (float32 only)", what, dtype);
  if (lengths != nullptr && lengths_dtype != RBX_I32 && lengths_dtype != RBX_I64)
    return fail(RBX_ERR_UNSUPPORTED, "%s: lengths_dtype=%d", what, lengths_dtype);
  if ((batch + kGruTile - 1) / kGruTile > INT_MAX)
    return fail(RBX_ERR_UNSUPPORTED, "%s: batch=%lld is too large", what, static_cast<long long>(batch));
  return RBX_OK;
}

// launch(KSMAX, CELL), both as integral constants, for the instantiation that serves (hidden, cell)
template <class F>
static void gru_instantiation(int32_t hidden, const int32_t* cell, F launch) {
  auto by_width = [&](auto c) {
    if (hidden <= 32) launch(std::integral_constant<int, 8>{}, c);
    else if (hidden <= 64) launch(std::integral_constant<int, 16>{}, c);
    else launch(std::integral_constant<int, 32>{}, c);
  };
  if (cell == nullptr) by_width(std::integral_constant<int, kGru>{});
  else if (*cell == kAugru) by_width(std::integral_constant<int, kAugru>{});
  else by_width(std::integral_constant<int, kAgru>{});
}

static int gru_fwd(const char* what, const int32_t* cell, const float* d_gi, int64_t gi_stride_b, int64_t gi_stride_t,
                   const float* d_att, const float* d_w_hh, const float* d_b_hh, const float* d_h0, const void* d_lengths,
                   int32_t lengths_dtype, int64_t batch, int32_t seq_len, int32_t hidden, int32_t dtype, float* d_out,
                   float* d_saved, float* d_hn, void* stream) {
  const int rc = gru_check(what, batch, seq_len, hidden, cell, dtype, d_lengths, lengths_dtype);
  if (rc != RBX_OK) return rc;
  if (batch == 0) return RBX_OK;
  if (!d_gi || (cell && !d_att) || !d_w_hh || !d_out || !d_saved || !d_hn) return fail(RBX_ERR_INVALID, "%s: NULL tensor", what);
  if (!aligned16(d_gi) || (gi_stride_b & 3) != 0 || (gi_stride_t & 3) != 0 || gi_stride_t < 3 * hidden)
    return fail(RBX_ERR_UNSUPPORTED, "%s: gi must be 16-byte aligned with strides that are multiples of 4 floats", what);
  const dim3 grid(static_cast<unsigned>((batch + kGruTile - 1) / kGruTile)), block(64 * ((hidden + 15) / 16));
  gru_instantiation(hidden, cell, [&](auto ks, auto c) {
    hipLaunchKernelGGL((gru_fwd_kernel<decltype(ks)::value, decltype(c)::value>), grid, block, 0, as_stream(stream), d_gi,
                       gi_stride_b, gi_stride_t, d_att, d_w_hh, d_b_hh, d_h0, d_lengths, lengths_dtype, batch, seq_len, hidden,
                       d_out, d_saved, d_hn);
  });
  return check_launch(what);
}

static int gru_bwd(const char* what, const int32_t* cell, const float* d_saved, const float* d_att, const float* d_w_hh,
                   const float* d_dout, int64_t dout_stride_b, int64_t dout_stride_t, const float* d_dhn, const void* d_lengths,
                   int32_t lengths_dtype, int64_t batch, int32_t seq_len, int32_t hidden, int32_t dtype, float* d_dgi,
                   float* d_dghn, float* d_datt, float* d_dh0, void* stream) {
  const int rc = gru_check(what, batch, seq_len, hidden, cell, dtype, d_lengths, lengths_dtype);
  if (rc != RBX_OK) return rc;
  if (batch == 0) return RBX_OK;
  if (!d_saved || (cell && (!d_att || !d_datt)) || !d_w_hh || !d_dgi || !d_dghn || !d_dh0)
    return fail(RBX_ERR_INVALID, "%s: NULL tensor", what);
  if (d_dout != nullptr && (!aligned16(d_dout) || (dout_stride_b & 3) != 0 || (dout_stride_t & 3) != 0 || dout_stride_t < hidden))
    return fail(RBX_ERR_UNSUPPORTED, "%s: d_out must be 16-byte aligned with strides that are multiples of 4 floats", what);
  const dim3 grid(static_cast<unsigned>((batch + kGruTile - 1) / kGruTile)), block(64 * ((hidden + 15) / 16));
  gru_instantiation(hidden, cell, [&](auto ks, auto c) {
    hipLaunchKernelGGL((gru_bwd_kernel<decltype(ks)::value, decltype(c)::value>), grid, block, 0, as_stream(stream), d_saved,
                       d_att, d_w_hh, d_dout, dout_stride_b, dout_stride_t, d_dhn, d_lengths, lengths_dtype, batch, seq_len,
                       hidden, d_dgi, d_dghn, d_datt, d_dh0);
  });
  return check_launch(what);
}

}  // namespace rbx

extern "C" int rbx_gru_supported(int32_t hidden, int32_t seq_len) {
  using namespace rbx;
  return seq_len >= 1 && hidden >= kGruMinH && hidden <= kGruMaxH && (hidden & 3) == 0;
}

extern "C" int rbx_attgru_supported(int32_t hidden, int32_t seq_len, int32_t cell) {
  return rbx_gru_supported(hidden, seq_len) && (cell == rbx::kAgru || cell == rbx::kAugru);
}

extern "C" int rbx_gru_fwd(const float* d_gi, int64_t gi_stride_b, int64_t gi_stride_t, const float* d_w_hh,
                           const float* d_b_hh, const float* d_h0, const void* d_lengths, int32_t lengths_dtype,
                           int64_t batch, int32_t seq_len, int32_t hidden, int32_t dtype, float* d_out, float* d_saved,
                           float* d_hn, void* stream) {
  return rbx::gru_fwd("gru_fwd", nullptr, d_gi, gi_stride_b, gi_stride_t, nullptr, d_w_hh, d_b_hh, d_h0, d_lengths,
                      lengths_dtype, batch, seq_len, hidden, dtype, d_out, d_saved, d_hn, stream);
}

extern "C" int rbx_gru_bwd(const float* d_saved, const float* d_w_hh, const float* d_dout, int64_t dout_stride_b,
                           int64_t dout_stride_t, const float* d_dhn, const void* d_lengths, int32_t lengths_dtype,
                           int64_t batch, int32_t seq_len, int32_t hidden, int32_t dtype, float* d_dgi, float* d_dghn,
                           float* d_dh0, void* stream) {
  return rbx::gru_bwd("gru_bwd", nullptr, d_saved, nullptr, d_w_hh, d_dout, dout_stride_b, dout_stride_t, d_dhn, d_lengths,
                      lengths_dtype, batch, seq_len, hidden, dtype, d_dgi, d_dghn, nullptr, d_dh0, stream);
}

extern "C" int rbx_attgru_fwd(const float* d_gi, int64_t gi_stride_b, int64_t gi_stride_t, const float* d_att,
                              const float* d_w_hh, const float* d_b_hh, const float* d_h0, const void* d_lengths,
                              int32_t lengths_dtype, int64_t batch, int32_t seq_len, int32_t hidden, int32_t cell,
                              int32_t dtype, float* d_out, float* d_saved, float* d_hn, void* stream) {
  return rbx::gru_fwd("attgru_fwd", &cell, d_gi, gi_stride_b, gi_stride_t, d_att, d_w_hh, d_b_hh, d_h0, d_lengths,
                      lengths_dtype, batch, seq_len, hidden, dtype, d_out, d_saved, d_hn, stream);
}

extern "C" int rbx_attgru_bwd(const float* d_saved, const float* d_att, const float* d_w_hh, const float* d_dout,
                              int64_t dout_stride_b, int64_t dout_stride_t, const float* d_dhn, const void* d_lengths,
                              int32_t lengths_dtype, int64_t batch, int32_t seq_len, int32_t hidden, int32_t cell,
                              int32_t dtype, float* d_dgi, float* d_dghn, float* d_datt, float* d_dh0, void* stream) {
  return rbx::gru_bwd("attgru_bwd", &cell, d_saved, d_att, d_w_hh, d_dout, dout_stride_b, dout_stride_t, d_dhn, d_lengths,
                      lengths_dtype, batch, seq_len, hidden, dtype, d_dgi, d_dghn, d_datt, d_dh0, stream);
}
