// rbx_addattn.hip -- additive attention pooling of the session-based matching models (gfx950, wave64).  Replaces the ATen lines
// of rechub's NARM (third_party/rechub/models/matching/narm.py:60-68, Eq. 6-8) and STAMP (stamp.py:69-72, Eq. 7-8):
//   q[b,l] = v . sigmoid(x[b,l] W^T + ctx[b])     e[b,l] = exp(q[b,l]) mask[b,l]  (as written: no max subtraction)
//   alpha[b,l] = e[b,l] / max(sum_l e[b,l], eps)   out[b] = sum_l alpha[b,l] x[b,l]
// x [B, L, D], W [H, D], ctx [B, H] (NULL = zeros), v [H], mask [B, L] (NULL = all valid).
//
// Both kernels: one workgroup walks samples b = blockIdx.x, blockIdx.x + gridDim.x, ...  It has ceil(max(D, H) / 16) wavefronts
// (1 .. 8); wavefront w owns hidden units 16 w .. 16 w + 15 and, in the backward, columns 16 w .. 16 w + 15 of dx.  Its slice of
// W is loaded ONCE into D / 4 B-operand registers per lane (W[unit][4 s + quad]) and stays there for all samples of the
// workgroup.  A sample is walked in tiles of 16 positions: the tile of x is staged in LDS k-major ([D][16 + 1]: the A operand
// of k-step s is rows 4 s .. 4 s + 3, conflict-free) and x W^T [16, 16 per wave] runs on v_mfma_f32_16x16x4_f32 (exact fp32;
// rows = positions, k = column of x, columns = the wave's units).  Nothing of size [B, L, H] is written by the forward.
//
// addattn_fwd_kernel  per tile: the accumulator lane that owns (unit j, positions 4 q .. 4 q + 3) forms v_j sigmoid(.), the 16
//                     units of a wave are summed by shuffles, the waves through LDS in wave order; e = exp(q) or 0 goes to
//                     alpha[b, l], its sum stays in registers.  Then alpha = e / max(sum, eps) as an IEEE division (one valid
//                     position gives exactly 1, k equal logits exactly 1.0f / k) and out = sum_l alpha_l x_l over the rows of x
//                     just read (they come from L2), four position groups added in a fixed order.
// addattn_bwd_kernel  G = sum_l alpha_l (dout . x_l) first; then per tile s = sigmoid(.) again on the MFMA, g_l = dout . x_l,
//                     dq_l = alpha_l (g_l - G), dpre = dq_l v_j s (1 - s): summed over l into dctx[b], dq_l s summed over l AND
//                     the workgroup's samples into one row of the workspace (dv), dpre itself written once to d_dpre [B, L, H]
//                     (a transient of the backward; the dense path forms dW = dpre^T x from it) and exchanged through a [H][16]
//                     LDS image for dx = alpha_l dout + dpre W: a second MFMA chain over k = hidden unit against the wave's
//                     H / 4 register-held B operands W[4 s + quad][column].
// addattn_dv_kernel   dv[h] = sum over the workgroups' rows, fixed order.
// No atomics, every sum in a fixed order: two runs give the same bits.  No host read-back; everything on the caller's stream.
#include "rbx_internal.h"

namespace rbx {

constexpr int kAaTile = 16;                 // positions per tile = rows of the MFMA
constexpr int kAaPad = kAaTile + 1;         // row stride of the staged x tile
constexpr int kAaMin = 4, kAaMax = 128;     // D and H
constexpr int kAaMaxGrid = 2048;            // workgroups of a launch = rows of the dv workspace

__device__ __forceinline__ bool aa_mask_on(const void* p, long long idx, int dt) {
  if (p == nullptr) return true;
  switch (dt) {
    case RBX_I32: return static_cast<const int*>(p)[idx] != 0;
    case RBX_I64: return static_cast<const long long*>(p)[idx] != 0;
    case RBX_F32: return static_cast<const float*>(p)[idx] != 0.f;
    default:      return static_cast<const unsigned char*>(p)[idx] != 0;
  }
}

// sum over the 16 lanes that share a quad (the 16 units / columns of a wave)

// rows l0 .. l0 + 15 of x[b] into xs[c * kAaPad + row]; zeros beyond L
__device__ __forceinline__ void aa_stage(const float* __restrict__ xb, const long long xs_l, const int l0, const int L,
                                         const int D, float* __restrict__ xs) {
  for (int i = threadIdx.x; i < kAaTile * D; i += blockDim.x) {
    const int row = i / D, c = i - row * D;
    xs[c * kAaPad + row] = (l0 + row < L) ? xb[(l0 + row) * xs_l + c] : 0.f;
  }
}

// KS = k-steps (of 4) the register file is laid out for: D <= 4 KS and H <= 4 KS; blockDim.x = 64 ceil(max(D, H) / 16)
template <int KS>
__global__ __launch_bounds__(16 * KS) void addattn_fwd_kernel(
    const float* __restrict__ x, const long long xs_b, const long long xs_l, const float* __restrict__ w,
    const float* __restrict__ ctx, const float* __restrict__ v, const void* __restrict__ mask, const int mask_dt,
    const float eps, const long long B, const int L, const int D, const int H, float* __restrict__ out,
    float* __restrict__ alpha) {
  __shared__ float xs[4 * KS * kAaPad];    // the x tile; afterwards the four partial sums of out [4][D]
  __shared__ float qp[KS / 4][kAaTile];    // per wave: the tile's partial logits
  __shared__ float den;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, col = lane & 15, quad = lane >> 4;
  const int j = wv * 16 + col;
  const bool jok = j < H;
  const int nkd = D >> 2, nwh = (H + 15) >> 4;

  float wf[KS];                            // B operand of k-step s: W[j, 4 s + quad]
#pragma unroll
  for (int s = 0; s < KS; ++s) wf[s] = (jok && s < nkd) ? w[j * D + 4 * s + quad] : 0.f;
  const float vj = jok ? v[j] : 0.f;

  for (long long b = blockIdx.x; b < B; b += gridDim.x) {
    const float* xb = x + b * xs_b;
    float* ab = alpha + b * L;
    const float cj = (ctx != nullptr && jok) ? ctx[b * H + j] : 0.f;
    float esum = 0.f;                      // threads 0 .. 15: the sum of e over the rows they own
    for (int l0 = 0; l0 < L; l0 += kAaTile) {
      aa_stage(xb, xs_l, l0, L, D, xs);
      __syncthreads();
      if (wv < nwh) {
        f32x4 acc = {cj, cj, cj, cj};
#pragma unroll
        for (int s = 0; s < KS; ++s)
          if (s < nkd) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xs[(4 * s + quad) * kAaPad + col], wf[s], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float t = group_sum<16, kWave>(vj * sigmoidf_fast(acc[r]));
          if (col == 0) qp[wv][quad * 4 + r] = t;
        }
      }
      __syncthreads();
      if (threadIdx.x < kAaTile && l0 + threadIdx.x < L) {
        float q = 0.f;
        for (int k = 0; k < nwh; ++k) q += qp[k][threadIdx.x];
        const float e = aa_mask_on(mask, b * L + l0 + threadIdx.x, mask_dt) ? expf(q) : 0.f;
        ab[l0 + threadIdx.x] = e;
        esum += e;
      }
    }
    if (wv == 0) {
      esum = group_sum<16, kWave>(esum);
      if (lane == 0) den = fmaxf(esum, eps);
    }
    __syncthreads();                       // den, and every e of this sample (written by this workgroup)
    const float d = den;
    for (int l = threadIdx.x; l < L; l += blockDim.x) ab[l] = ab[l] / d;
    __syncthreads();
    // out: thread (group g = tid / D < 4, column c) sums positions g, g + 4, ...; the four groups are added in order
    const int g = threadIdx.x / D, c = threadIdx.x - g * D;
    if (g < 4) {
      float o = 0.f;
      for (int l = g; l < L; l += 4) o = fma_rn(ab[l], xb[l * xs_l + c], o);
      xs[g * D + c] = o;
    }
    __syncthreads();
    if (threadIdx.x < D) out[b * D + threadIdx.x] = ((xs[threadIdx.x] + xs[D + threadIdx.x]) + xs[2 * D + threadIdx.x]) +
                                                   xs[3 * D + threadIdx.x];
    __syncthreads();                       // xs is staged again for the next sample
  }
}

template <int KS>
__global__ __launch_bounds__(16 * KS) void addattn_bwd_kernel(
    const float* __restrict__ dout, const long long ds_b, const float* __restrict__ x, const long long xs_b,
    const long long xs_l, const float* __restrict__ w, const float* __restrict__ ctx, const float* __restrict__ v,
    const float* __restrict__ alpha, const long long B, const int L, const int D, const int H, float* __restrict__ dx,
    float* __restrict__ dctx, float* __restrict__ dvp, float* __restrict__ dpre) {
  __shared__ float xs[4 * KS * kAaPad];                               // the x tile [D][17]
  __shared__ __attribute__((aligned(16))) float dp[4 * KS * kAaTile]; // dpre of the tile [H][16]
  __shared__ float dd[4 * KS];                                        // dout[b]
  __shared__ float gw[KS / 4];                                        // per wave: its share of G
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, col = lane & 15, quad = lane >> 4;
  const int j = wv * 16 + col;             // the hidden unit of the first chain, the column of dx of the second
  const bool jok = j < H, cok = j < D;
  const int nkd = D >> 2, nkh = H >> 2, nwh = (H + 15) >> 4, nwd = (D + 15) >> 4, nw = blockDim.x >> 6;

  float wf[KS], wt[KS];                    // B operands: W[j, 4 s + quad] (k = column of x); W[4 s + quad, j] (k = unit)
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    wf[s] = (jok && s < nkd) ? w[j * D + 4 * s + quad] : 0.f;
    wt[s] = (cok && s < nkh) ? w[(4 * s + quad) * D + j] : 0.f;
  }
  const float vj = jok ? v[j] : 0.f;
  float dv_acc = 0.f;                      // sum over positions 4 q .. 4 q + 3 of every tile of every sample: dq s

  for (long long b = blockIdx.x; b < B; b += gridDim.x) {
    const float* xb = x + b * xs_b;
    const float* ab = alpha + b * L;
    const float cj = (ctx != nullptr && jok) ? ctx[b * H + j] : 0.f;
    if (threadIdx.x < D) dd[threadIdx.x] = dout[b * ds_b + threadIdx.x];
    __syncthreads();
    // G = sum_l alpha_l g_l: quad q of wave w takes positions 4 w + q, 4 (w + nw) + q, ...; the quads, then the waves, are
    // added in order.  g_l = dout . x_l is summed exactly as the tile loop below sums it (this lane's columns col, col + 16,
    // ..., then the 16 lanes), so g_l - G cancels to the bit where one position holds all the weight: its dq is 0, not the
    // rounding of two summation orders
    float gpart = 0.f;
    for (int l0 = wv * 4; l0 < L; l0 += 4 * nw) {
      const int l = l0 + quad;
      float p = 0.f;
      if (l < L)
        for (int c = col; c < D; c += 16) p = fma_rn(dd[c], xb[l * xs_l + c], p);
      gpart = fma_rn(l < L ? ab[l] : 0.f, group_sum<16, kWave>(p), gpart);
    }
    gpart += __shfl_xor(gpart, 16, 64);
    gpart += __shfl_xor(gpart, 32, 64);
    if (lane == 0) gw[wv] = gpart;
    __syncthreads();
    float G = 0.f;
    for (int k = 0; k < nw; ++k) G += gw[k];

    float dc_acc = 0.f;                    // sum over this sample's positions 4 q + r of dpre (unit j)
    for (int l0 = 0; l0 < L; l0 += kAaTile) {
      aa_stage(xb, xs_l, l0, L, D, xs);
      __syncthreads();
      float al[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) al[r] = (l0 + quad * 4 + r < L) ? ab[l0 + quad * 4 + r] : 0.f;
      if (wv < nwh) {
        f32x4 acc = {cj, cj, cj, cj};
#pragma unroll
        for (int s = 0; s < KS; ++s)
          if (s < nkd) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xs[(4 * s + quad) * kAaPad + col], wf[s], acc, 0, 0, 0);
        float dpr[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = quad * 4 + r;
          float p = 0.f;                   // g_l = dout . x_l: this lane's columns col, col + 16, ..., then the 16 lanes
          for (int c = col; c < D; c += 16) p = fma_rn(dd[c], xs[c * kAaPad + row], p);
          const float dq = al[r] * (group_sum<16, kWave>(p) - G);
          const float sg = sigmoidf_fast(acc[r]);
          dpr[r] = jok ? dq * vj * sg * (1.f - sg) : 0.f;
          dc_acc += dpr[r];
          dv_acc += jok ? dq * sg : 0.f;
          if (dpre != nullptr && jok && l0 + row < L) dpre[(b * L + l0 + row) * H + j] = dpr[r];
        }
        if (jok) *reinterpret_cast<float4*>(&dp[j * kAaTile + quad * 4]) = make_float4(dpr[0], dpr[1], dpr[2], dpr[3]);
      }
      __syncthreads();                     // dpre of the tile is in dp; nobody reads xs any more
      if (wv < nwd) {
        const float dj = cok ? dd[j] : 0.f;
        f32x4 acc = {al[0] * dj, al[1] * dj, al[2] * dj, al[3] * dj};
#pragma unroll
        for (int s = 0; s < KS; ++s)
          if (s < nkh) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(dp[64 * s + lane], wt[s], acc, 0, 0, 0);
        if (cok) {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (l0 + quad * 4 + r < L) dx[(b * L + l0 + quad * 4 + r) * D + j] = acc[r];
        }
      }
    }
    dc_acc += __shfl_xor(dc_acc, 16, 64);
    dc_acc += __shfl_xor(dc_acc, 32, 64);
    if (jok && quad == 0) dctx[b * H + j] = dc_acc;
    __syncthreads();                       // dd, gw, xs and dp are written again for the next sample
  }
  dv_acc += __shfl_xor(dv_acc, 16, 64);
  dv_acc += __shfl_xor(dv_acc, 32, 64);
  if (jok && quad == 0) dvp[static_cast<long long>(blockIdx.x) * H + j] = dv_acc;
}

// dv[h] = sum_g part[g, h]: thread (row lane r = tid / 16, column tid % 16) adds rows r, r + 16, ..., then a tree over the lanes
__global__ __launch_bounds__(256) void addattn_dv_kernel(const float* __restrict__ part, const int rows, const int H,
                                                         float* __restrict__ dv) {
  __shared__ float sm[16][17];
  const int c = threadIdx.x & 15, r = threadIdx.x >> 4, h = blockIdx.x * 16 + c;
  float s = 0.f;
  if (h < H)
    for (int g = r; g < rows; g += 16) s += part[static_cast<long long>(g) * H + h];
  sm[r][c] = s;
  __syncthreads();
  for (int o = 8; o > 0; o >>= 1) {
    if (r < o) sm[r][c] += sm[r + o][c];
    __syncthreads();
  }
  if (r == 0 && h < H) dv[h] = sm[0][c];
}

static unsigned aa_grid(int64_t batch) { return static_cast<unsigned>(batch < kAaMaxGrid ? batch : kAaMaxGrid); }

static int aa_check(const char* what, int64_t batch, int32_t seq_len, int32_t dim, int32_t hidden, int32_t dtype,
                    const void* mask, int32_t mask_dtype, const void* x, int64_t xs_b, int64_t xs_l) {
  if (batch < 0) return fail(RBX_ERR_INVALID, "%s: batch=%lld", what, static_cast<long long>(batch));
  if (!rbx_addattn_supported(dim, hidden, seq_len))
    return fail(RBX_ERR_UNSUPPORTED, "%s: dim=%d and hidden=%d must be multiples of 4 in [%d,%d], seq_len=%d >= 1", what, dim,
                hidden, kAaMin, kAaMax, seq_len);
  if (dtype != RBX_F32) return fail(RBX_ERR_UNSUPPORTED, "%s: tensor dtype code %d (float32 only)", what, dtype);
  if (mask != nullptr && mask_dtype != RBX_I32 && mask_dtype != RBX_I64 && mask_dtype != RBX_F32 && mask_dtype != RBX_MASK_U8)
    return fail(RBX_ERR_UNSUPPORTED, "%s: mask_dtype=%d", what, mask_dtype);
  if (x != nullptr && (!aligned16(x) || (xs_b & 3) != 0 || (xs_l & 3) != 0 || xs_l < dim || xs_b < 0))
    return fail(RBX_ERR_UNSUPPORTED, "%s: x must be 16-byte aligned with strides that are multiples of 4 floats", what);
  return RBX_OK;
}

}  // namespace rbx

extern "C" int rbx_addattn_supported(int32_t dim, int32_t hidden, int32_t seq_len) {
  using namespace rbx;
  return seq_len >= 1 && dim >= kAaMin && dim <= kAaMax && (dim & 3) == 0 && hidden >= kAaMin && hidden <= kAaMax &&
         (hidden & 3) == 0;
}

#define RBX_AA_DISPATCH(KERNEL, ...)                                                                    \
  do {                                                                                                  \
    const int widest = dim > hidden ? dim : hidden;                                                     \
    const dim3 grid(aa_grid(batch)), block(64 * ((widest + 15) / 16));                                  \
    if (widest <= 32) hipLaunchKernelGGL(KERNEL<8>, grid, block, 0, s, __VA_ARGS__);                    \
    else if (widest <= 64) hipLaunchKernelGGL(KERNEL<16>, grid, block, 0, s, __VA_ARGS__);              \
    else hipLaunchKernelGGL(KERNEL<32>, grid, block, 0, s, __VA_ARGS__);                                \
  } while (0)

extern "C" int rbx_addattn_fwd(const float* d_x, int64_t x_stride_b, int64_t x_stride_l, const float* d_w, const float* d_ctx,
                               const float* d_v, const void* d_mask, int32_t mask_dtype, float eps, int64_t batch,
                               int32_t seq_len, int32_t dim, int32_t hidden, int32_t dtype, float* d_out, float* d_alpha,
                               void* stream) {
  using namespace rbx;
  const int rc = aa_check("addattn_fwd", batch, seq_len, dim, hidden, dtype, d_mask, mask_dtype, d_x, x_stride_b, x_stride_l);
  if (rc != RBX_OK) return rc;
  if (batch == 0) return RBX_OK;
  if (!d_x || !d_w || !d_v || !d_out || !d_alpha) return fail(RBX_ERR_INVALID, "addattn_fwd: NULL tensor");
  hipStream_t s = as_stream(stream);
  RBX_AA_DISPATCH(addattn_fwd_kernel, d_x, x_stride_b, x_stride_l, d_w, d_ctx, d_v, d_mask, mask_dtype, eps, batch, seq_len,
                  dim, hidden, d_out, d_alpha);
  return check_launch("addattn_fwd");
}

extern "C" size_t rbx_addattn_bwd_workspace_size(int64_t batch, int32_t hidden) {
  if (batch <= 0 || hidden <= 0) return 0;
  return static_cast<size_t>(rbx::aa_grid(batch)) * hidden * sizeof(float);
}

extern "C" int rbx_addattn_bwd(const float* d_dout, int64_t dout_stride_b, const float* d_x, int64_t x_stride_b,
                               int64_t x_stride_l, const float* d_w, const float* d_ctx, const float* d_v, const void* d_mask,
                               int32_t mask_dtype, const float* d_alpha, float eps, int64_t batch, int32_t seq_len, int32_t dim,
                               int32_t hidden, int32_t dtype, float* d_dx, float* d_dctx, float* d_dv, float* d_dpre,
                               void* d_workspace, size_t workspace_bytes, void* stream) {
  using namespace rbx;
  (void)eps;                               // alpha carries the mask and the clamp: a row that was clamped has alpha = 0
  const int rc = aa_check("addattn_bwd", batch, seq_len, dim, hidden, dtype, d_mask, mask_dtype, d_x, x_stride_b, x_stride_l);
  if (rc != RBX_OK) return rc;
  if (batch == 0) return RBX_OK;
  if (!d_dout || !d_x || !d_w || !d_v || !d_alpha || !d_dx || !d_dctx || !d_dv)
    return fail(RBX_ERR_INVALID, "addattn_bwd: NULL tensor");
  if (!aligned16(d_dout) || (dout_stride_b & 3) != 0 || dout_stride_b < dim)
    return fail(RBX_ERR_UNSUPPORTED, "addattn_bwd: d_out must be 16-byte aligned with a row stride that is a multiple of 4 floats");
  if (d_workspace == nullptr || workspace_bytes < rbx_addattn_bwd_workspace_size(batch, hidden))
    return fail(RBX_ERR_WORKSPACE, "addattn_bwd: workspace too small");
  hipStream_t s = as_stream(stream);
  float* part = static_cast<float*>(d_workspace);
  RBX_AA_DISPATCH(addattn_bwd_kernel, d_dout, dout_stride_b, d_x, x_stride_b, x_stride_l, d_w, d_ctx, d_v, d_alpha, batch,
                  seq_len, dim, hidden, d_dx, d_dctx, part, d_dpre);
  hipLaunchKernelGGL(addattn_dv_kernel, dim3((hidden + 15) / 16), dim3(256), 0, s, part, static_cast<int>(aa_grid(batch)),
                     hidden, d_dv);
  return check_launch("addattn_bwd");
}
#undef RBX_AA_DISPATCH
