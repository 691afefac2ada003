// rbx_inbatch.hip -- in-batch negatives: the band of the [B, B] cosine matrix that YoutubeSBC keeps (gfx950, wave64).  Replaces,
// under third_party/rechub/models/matching/youtube_sbc.py, torch.cosine_similarity(user.unsqueeze(1), item, dim=2) -- a
// [B, B, D] broadcast -- minus log(sample_weight) and the [index0, index1] gather of B (n_neg + 1) of its B B entries.
// u, v [B, D] read with a row stride, w [B] optional, j = (i + k) mod B, k = 0 .. n_neg:
//
//   ru_i = 1 / max(|u_i|, eps)      rv_j = 1 / max(|v_j|, eps)      scores[i, k] = (<u_i, v_j> ru_i rv_j - log w_j) inv_temperature
//
// ib_fwd_kernel  a workgroup of 256 threads takes kIbTile = 16 consecutive rows, one lane group of 16 lanes per row.  It stages
//                its 16 user rows and the 16 + n_neg item rows its band touches (wrapped through mod B) in LDS once, with float4
//                loads; the lane groups form the norms of the staged rows and then the n_neg + 1 dots of their row from LDS.
//                ru and rv are written for the backward (rv by the tile that owns the row).
// ib_bwd_kernel  the same tile for du_i (over the row's own band) and for dv_j, dw_j (over the mirrored band, users
//                (j - k) mod B): stages the n_neg + 16 user rows, their g rows and the 16 + n_neg item rows, recomputes the
//                cosines of every pair it needs into LDS and gathers.  A clamped norm is a constant denominator.
// No atomics, every sum in ascending k: two runs give the same bits.  No MFMA: D FLOP per 8 staged bytes.  No call allocates or
// synchronises.
#include <math.h>

#include "rbx_internal.h"

namespace rbx {

constexpr int kIbTile = 16;                  // rows per workgroup = lane groups per workgroup
constexpr int kIbGroup = 16;                 // lanes per row
constexpr int kIbBlock = kIbTile * kIbGroup;
constexpr int kIbMaxDim = 512;
constexpr int kIbMaxNeg = 64;                // and what the backward's LDS image admits at this D: ib_max_neg
constexpr size_t kIbLdsCap = 160 * 1024;

// floats of LDS: forward = user tile + item halo + the halo's inverse norms; backward = both halos, the g and cosine rows of the
// user halo, both inverse norms
static size_t ib_fwd_lds(int D, int n) { return sizeof(float) * (static_cast<size_t>(kIbTile) * D + static_cast<size_t>(kIbTile + n) * (D + 1)); }
static size_t ib_bwd_lds(int D, int n) { return sizeof(float) * static_cast<size_t>(kIbTile + n) * (2 * D + 2 * (n + 1) + 2); }

static int ib_max_neg(int D) {
  int n = kIbMaxNeg;
  while (n > 0 && ib_bwd_lds(D, n) > kIbLdsCap) --n;
  return n;
}

struct IbArgs {
  const float *u, *v, *w;    // u[i us + c], v[j vs + c], w[j] or NULL
  long long us, vs;
  float* scores;             // forward: scores[i ss + k]
  long long ss;
  float *ru, *rv;            // [B]: written by the forward, read by the backward
  const float* g;            // backward: g[i gs + k]
  long long gs;
  float *du, *dv, *dw;       // any of them NULL: not wanted
  long long dus, dvs;
  long long B;
  int D, n;
  float eps, inv_t;
};

__device__ __forceinline__ long long ib_wrap(long long x, long long B) {
  const long long m = x % B;
  return m < 0 ? m + B : m;
}

// rows[slot][:] = src[wrap(first + slot)][:] for slot < count, float4 by float4
__device__ __forceinline__ void ib_stage(float* rows, const float* src, long long stride, long long first, int count, int D4,
                                         long long B) {
  for (int e = threadIdx.x; e < count * D4; e += kIbBlock) {
    const int t = e / D4, c = e - t * D4;
    const long long r = ib_wrap(first + t, B);
    reinterpret_cast<float4*>(rows)[e] = *reinterpret_cast<const float4*>(src + r * stride + 4 * c);
  }
}

__device__ __forceinline__ float ib_dot(const float* x, const float* y, int D4, int lane) {
  float s = 0.f;
  for (int c = lane; c < D4; c += kIbGroup) {
    const float4 a = reinterpret_cast<const float4*>(x)[c], b = reinterpret_cast<const float4*>(y)[c];
    s += a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w;
  }
  return group_sum<kIbGroup>(s);
}

__global__ __launch_bounds__(kIbBlock) void ib_fwd_kernel(const IbArgs a) {
  extern __shared__ __attribute__((aligned(16))) float ib_lds[];
  const int D = a.D, n = a.n, D4 = D >> 2, H = kIbTile + n;
  float* us = ib_lds;                        // [16][D]   rows r0 ..
  float* vs = us + kIbTile * D;              // [H][D]    rows (r0 + s) mod B
  float* rvs = vs + H * D;                   // [H]
  const long long B = a.B, r0 = static_cast<long long>(blockIdx.x) * kIbTile;
  const int group = threadIdx.x >> 4, lane = threadIdx.x & (kIbGroup - 1);
  ib_stage(us, a.u, a.us, r0, kIbTile, D4, B);
  ib_stage(vs, a.v, a.vs, r0, H, D4, B);
  __syncthreads();
  for (int s = group; s < H; s += kIbTile) {
    const float inv = 1.f / fmaxf(sqrtf(ib_dot(vs + s * D, vs + s * D, D4, lane)), a.eps);
    if (lane == 0) {
      rvs[s] = inv;
      if (s < kIbTile && r0 + s < B) a.rv[r0 + s] = inv;
    }
  }
  const float* urow = us + group * D;
  const float ru = 1.f / fmaxf(sqrtf(ib_dot(urow, urow, D4, lane)), a.eps);
  __syncthreads();
  const long long i = r0 + group;
  if (i >= B) return;
  if (lane == 0) a.ru[i] = ru;
  for (int k = 0; k <= n; ++k) {
    const float d = ib_dot(urow, vs + (group + k) * D, D4, lane);
    if (lane == 0) {
      const float lw = a.w != nullptr ? logf(a.w[ib_wrap(i + k, B)]) : 0.f;
      a.scores[i * a.ss + k] = (d * ru * rvs[group + k] - lw) * a.inv_t;
    }
  }
}

__global__ __launch_bounds__(kIbBlock) void ib_bwd_kernel(const IbArgs a) {
  extern __shared__ __attribute__((aligned(16))) float ib_lds[];
  const int D = a.D, n = a.n, n1 = n + 1, D4 = D >> 2, H = kIbTile + n;
  float* us = ib_lds;                        // [H][D]    slot t: row (r0 - n + t) mod B; the tile's own rows are t = n ..
  float* vs = us + H * D;                    // [H][D]    slot s: row (r0 + s) mod B; the tile's own rows are s < 16
  float* gs = vs + H * D;                    // [H][n1]   g of the user slots
  float* cs = gs + H * n1;                   // [H][n1]   cosine of (user slot t, item slot t - n + k)
  float* rus = cs + H * n1;                  // [H]
  float* rvs = rus + H;                      // [H]
  const long long B = a.B, r0 = static_cast<long long>(blockIdx.x) * kIbTile;
  const int group = threadIdx.x >> 4, lane = threadIdx.x & (kIbGroup - 1);
  ib_stage(us, a.u, a.us, r0 - n, H, D4, B);
  ib_stage(vs, a.v, a.vs, r0, H, D4, B);
  for (int e = threadIdx.x; e < H * n1; e += kIbBlock) {
    const int t = e / n1, k = e - t * n1;
    gs[e] = a.g[ib_wrap(r0 - n + t, B) * a.gs + k];
  }
  for (int t = threadIdx.x; t < H; t += kIbBlock) {
    rus[t] = a.ru[ib_wrap(r0 - n + t, B)];
    rvs[t] = a.rv[ib_wrap(r0 + t, B)];
  }
  __syncthreads();
  // the pairs some row of this tile sums over: every k of the tile's own users (t >= n), and of the users before them the
  // pairs whose item is one of the tile's (s < 16)
  for (int p = group; p < H * n1; p += kIbTile) {
    const int t = p / n1, k = p - t * n1, s = t - n + k;
    if (s < 0 || (t < n && s >= kIbTile)) continue;
    const float d = ib_dot(us + t * D, vs + s * D, D4, lane);
    if (lane == 0) cs[p] = d * rus[t] * rvs[s];
  }
  __syncthreads();
  const long long row = r0 + group;
  if (row >= B) return;
  const float clamp = 1.f / a.eps;           // what the forward stored for a norm under eps
  if (a.du != nullptr) {
    const int t = n + group;
    const float ru = rus[t];
    float sg = 0.f;
    for (int k = 0; k <= n; ++k) sg += gs[t * n1 + k] * cs[t * n1 + k];
    const float self = ru >= clamp ? 0.f : ru * sg;
    for (int c = lane; c < D4; c += kIbGroup) {
      float4 acc = {0.f, 0.f, 0.f, 0.f};
      for (int k = 0; k <= n; ++k) {
        const float f = gs[t * n1 + k] * rvs[group + k];
        const float4 x = reinterpret_cast<const float4*>(vs + (group + k) * D)[c];
        acc.x += f * x.x; acc.y += f * x.y; acc.z += f * x.z; acc.w += f * x.w;
      }
      const float4 x = reinterpret_cast<const float4*>(us + t * D)[c];
      const float m = a.inv_t * ru;
      float4 o = {m * (acc.x - self * x.x), m * (acc.y - self * x.y), m * (acc.z - self * x.z), m * (acc.w - self * x.w)};
      *reinterpret_cast<float4*>(a.du + row * a.dus + 4 * c) = o;
    }
  }
  if (a.dv != nullptr || a.dw != nullptr) {
    const int s = group;
    const float rv = rvs[s];
    float sg = 0.f, sum = 0.f;
    for (int k = 0; k <= n; ++k) {
      const int t = s + n - k;
      sg += gs[t * n1 + k] * cs[t * n1 + k];
      sum += gs[t * n1 + k];
    }
    if (a.dw != nullptr && lane == 0) a.dw[row] = -a.inv_t * sum / a.w[row];
    if (a.dv != nullptr) {
      const float self = rv >= clamp ? 0.f : rv * sg;
      for (int c = lane; c < D4; c += kIbGroup) {
        float4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k <= n; ++k) {
          const int t = s + n - k;
          const float f = gs[t * n1 + k] * rus[t];
          const float4 x = reinterpret_cast<const float4*>(us + t * D)[c];
          acc.x += f * x.x; acc.y += f * x.y; acc.z += f * x.z; acc.w += f * x.w;
        }
        const float4 x = reinterpret_cast<const float4*>(vs + s * D)[c];
        const float m = a.inv_t * rv;
        float4 o = {m * (acc.x - self * x.x), m * (acc.y - self * x.y), m * (acc.z - self * x.z), m * (acc.w - self * x.w)};
        *reinterpret_cast<float4*>(a.dv + row * a.dvs + 4 * c) = o;
      }
    }
  }
}

static bool ib_rows_ok(const void* p, int64_t stride, int D) {
  return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && stride >= D && (stride & 3) == 0;
}

// the checks both entry points share; RBX_OK with *launch = false for an empty batch
static int ib_check(const char* what, const float* u, int64_t us, const float* v, int64_t vs, int64_t batch, int32_t dim,
                    int32_t n_neg, float eps, int32_t dtype, bool* launch) {
  *launch = false;
  if (batch < 0) return fail(RBX_ERR_INVALID, "%s: batch=%lld", what, (long long)batch);
  if (!rbx_inbatch_band_supported(dim, n_neg, dtype))
    return fail(RBX_ERR_UNSUPPORTED, "%s: dim=%d n_neg=%d dtype=%d (float32, dim a multiple of 4 up to %d, 1 <= n_neg <= %d at this "
                "dim)", what, dim, n_neg, dtype, kIbMaxDim, (dim >= 4 && dim <= kIbMaxDim) ? ib_max_neg(dim) : 0);
  if (batch == 0) return RBX_OK;
  if (n_neg >= batch) return fail(RBX_ERR_UNSUPPORTED, "%s: n_neg=%d needs a batch above it (batch=%lld)", what, n_neg, (long long)batch);
  if (!(eps > 0.f)) return fail(RBX_ERR_INVALID, "%s: eps must be positive", what);
  if (u == nullptr || v == nullptr) return fail(RBX_ERR_INVALID, "%s: NULL input", what);
  if (!ib_rows_ok(u, us, dim) || !ib_rows_ok(v, vs, dim))
    return fail(RBX_ERR_INVALID, "%s: u and v need 16-byte aligned rows (base and a row stride that is a multiple of 4, >= dim)", what);
  *launch = true;
  return RBX_OK;
}

}  // namespace rbx

extern "C" int rbx_inbatch_band_max_neg(int32_t dim) {
  if (dim < 4 || dim > rbx::kIbMaxDim || dim % 4 != 0) return 0;
  return rbx::ib_max_neg(dim);
}

extern "C" int rbx_inbatch_band_supported(int32_t dim, int32_t n_neg, int32_t dtype) {
  if (dtype != RBX_F32) return 0;
  return n_neg >= 1 && n_neg <= rbx_inbatch_band_max_neg(dim);
}

extern "C" int rbx_inbatch_band_fwd(const float* d_u, int64_t u_stride, const float* d_v, int64_t v_stride, const float* d_w,
                                    int64_t batch, int32_t dim, int32_t n_neg, float eps, float inv_temperature, int32_t dtype,
                                    float* d_scores, int64_t scores_stride, float* d_ru, float* d_rv, void* stream) {
  using namespace rbx;
  bool launch;
  const int rc = ib_check("inbatch_band_fwd", d_u, u_stride, d_v, v_stride, batch, dim, n_neg, eps, dtype, &launch);
  if (rc != RBX_OK || !launch) return rc;
  if (d_scores == nullptr || d_ru == nullptr || d_rv == nullptr) return fail(RBX_ERR_INVALID, "inbatch_band_fwd: NULL output");
  if (scores_stride < n_neg + 1) return fail(RBX_ERR_INVALID, "inbatch_band_fwd: scores_stride=%lld < n_neg + 1", (long long)scores_stride);
  IbArgs a{};
  a.u = d_u; a.v = d_v; a.w = d_w; a.us = u_stride; a.vs = v_stride; a.scores = d_scores; a.ss = scores_stride;
  a.ru = d_ru; a.rv = d_rv; a.B = batch; a.D = dim; a.n = n_neg; a.eps = eps; a.inv_t = inv_temperature;
  const size_t lds = ib_fwd_lds(dim, n_neg);
  const int rc_lds = allow_lds("inbatch_band_fwd", ib_fwd_kernel, lds);
  if (rc_lds != RBX_OK) return rc_lds;
  hipLaunchKernelGGL(ib_fwd_kernel, dim3(static_cast<unsigned>((batch + kIbTile - 1) / kIbTile)), dim3(kIbBlock), lds,
                     as_stream(stream), a);
  return check_launch("inbatch_band_fwd");
}

extern "C" int rbx_inbatch_band_bwd(const float* d_g, int64_t g_stride, const float* d_u, int64_t u_stride, const float* d_v,
                                    int64_t v_stride, const float* d_w, const float* d_ru, const float* d_rv, int64_t batch,
                                    int32_t dim, int32_t n_neg, float eps, float inv_temperature, int32_t dtype, float* d_du,
                                    int64_t du_stride, float* d_dv, int64_t dv_stride, float* d_dw, void* stream) {
  using namespace rbx;
  bool launch;
  const int rc = ib_check("inbatch_band_bwd", d_u, u_stride, d_v, v_stride, batch, dim, n_neg, eps, dtype, &launch);
  if (rc != RBX_OK || !launch) return rc;
  if (d_g == nullptr || d_ru == nullptr || d_rv == nullptr) return fail(RBX_ERR_INVALID, "inbatch_band_bwd: NULL input");
  if (g_stride < n_neg + 1) return fail(RBX_ERR_INVALID, "inbatch_band_bwd: g_stride=%lld < n_neg + 1", (long long)g_stride);
  if ((d_du != nullptr && !ib_rows_ok(d_du, du_stride, dim)) || (d_dv != nullptr && !ib_rows_ok(d_dv, dv_stride, dim)))
    return fail(RBX_ERR_INVALID, "inbatch_band_bwd: du and dv need 16-byte aligned rows");
  if (d_dw != nullptr && d_w == nullptr) return fail(RBX_ERR_INVALID, "inbatch_band_bwd: dw asked for without w");
  if (d_du == nullptr && d_dv == nullptr && d_dw == nullptr) return RBX_OK;
  IbArgs a{};
  a.u = d_u; a.v = d_v; a.w = d_w; a.us = u_stride; a.vs = v_stride; a.ru = const_cast<float*>(d_ru); a.rv = const_cast<float*>(d_rv);
  a.g = d_g; a.gs = g_stride; a.du = d_du; a.dv = d_dv; a.dw = d_dw; a.dus = du_stride; a.dvs = dv_stride;
  a.B = batch; a.D = dim; a.n = n_neg; a.eps = eps; a.inv_t = inv_temperature;
  const size_t lds = ib_bwd_lds(dim, n_neg);
  const int rc_lds = allow_lds("inbatch_band_bwd", ib_bwd_kernel, lds);
  if (rc_lds != RBX_OK) return rc_lds;
  hipLaunchKernelGGL(ib_bwd_kernel, dim3(static_cast<unsigned>((batch + kIbTile - 1) / kIbTile)), dim3(kIbBlock), lds,
                     as_stream(stream), a);
  return check_launch("inbatch_band_bwd");
}
