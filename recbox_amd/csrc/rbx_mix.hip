// rbx_mix.hip -- mixing expert outputs under per-task gates (gfx950, wave64): the step MMOE, CGC / PLE and AITM's AttentionLayer
// are named after.  Replaces, in rechub's multi-task models (third_party/rechub/models/multi_task/mmoe.py:46-57, ple.py:102-128,
// aitm.py:77-84), torch.cat of the E expert outputs into [B, E, H], one torch.mul per gate that writes another [B, E, H] (and
// that autograd keeps), and a torch.sum.
//
//   p_t[b, j]   = softmax_j(z_t[b, j])  (max-subtracted, fp32)    or    z_t[b, j]  (softmax = 0)
//   out_t[b, :] = sum_j p_t[b, j] X_{sel_t[j]}[b, :]
//
// Gate t mixes its own selection sel_t of the E experts (PLE: "own specific + shared"; its shared gate: all of them); the
// experts are separate tensors read through a pointer and a row stride each (AITM: two interleaved rows of one [B, 2, dim]).
// Everything a launch needs (pointers, strides, selections) travels by value in the kernel's argument struct (MixArgs, < 1 KiB):
// no device-side tables, no workspace, nothing on the stream but the launch.
//
// Both kernels make ONE pass over the experts for all T gates: lanes run along H as float4, X_e[b, :] is loaded once and used
// by every gate that selects e (the host turns the selections into pos[e] = position of e in each gate's selection, one byte per
// gate, 0xFF = not selected).  A sample is owned by a lane group of G = 1, 2, .. 64 lanes (G = H / 4 rounded up to a power of
// two; 64 / G samples per wavefront); from H = 260 on a lane owns NC = 2, 3, 4 float4 columns 64 apart.  The terms of out_t are
// added in ascending order of the expert index (= ascending j for an ascending selection), the terms of dX_e in ascending order
// of the gate.
//
// mix_fwd_kernel<NC>     per gate: running max and sum of exp over its logits (every lane of the group, the loads are
//                        broadcasts), then the expert loop; lane 0 of the group stores p [B, sum n_t] for the backward.
// mix_bwd_kernel<G, NC>  dout_t[b, :] of every gate is held in registers; per expert: dX_e = sum_t p dout_t and, per selecting
//                        gate, dp = <dout_t, X_e> reduced by wave shuffles inside the lane group.  softmax: lane j mod G of the
//                        group parks dp in dz_t[b, j] and, after the loop, rewrites its own entries as p (dp - s_t),
//                        s_t = sum_i p_i dp_i accumulated on the way (a lane reads back only what it wrote itself).
// No atomics, no LDS, every sum in a fixed order: two runs give the same bits.
#include "rbx_internal.h"

namespace rbx {

constexpr int kMixMaxE = 16, kMixMaxT = 8, kMixMaxN = 16;
constexpr int kMixMinH = 4, kMixMaxH = 1024;
constexpr int kMixBlock = 256;

struct MixArgs {
  const float* x[kMixMaxE];          // expert rows, read at x[e][b xs[e] + c]
  long long xs[kMixMaxE];
  const float* z[kMixMaxT];          // gate inputs [B, n_t]
  const float* g[kMixMaxT];          // backward: dout_t [B, H] or NULL (= zeros)
  float* dx[kMixMaxE];               // backward: dX_e [B, H] or NULL (= not wanted)
  float* dz[kMixMaxT];               // backward: dz_t [B, n_t] or NULL
  unsigned long long pos[kMixMaxE];  // byte t of pos[e]: position of e in gate t's selection, 0xFF = not selected
  int off[kMixMaxT + 1];             // gate t owns columns off[t] .. off[t + 1] of p
  float* out;                        // forward: [T, B, H]
  float* p;                          // [B, off[T]] (softmax only): written by the forward, read by the backward
  long long B;
  int H4, E, T, softmax, lg;         // H / 4; lg = log2(G)
};

__device__ __forceinline__ int mix_pos(unsigned long long pk, int t) { return static_cast<int>((pk >> (8 * t)) & 0xFFu); }

template <int NC>
__global__ __launch_bounds__(kMixBlock) void mix_fwd_kernel(const MixArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lig = lane & ((1 << a.lg) - 1);
  const long long b = (static_cast<long long>(blockIdx.x) * (kMixBlock / 64) + wave) * (64 >> a.lg) + (lane >> a.lg);
  const bool row = b < a.B;
  bool ok[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) ok[c] = row && lig + 64 * c < a.H4;

  float m[kMixMaxT], inv[kMixMaxT];
#pragma unroll
  for (int t = 0; t < kMixMaxT; ++t) {
    m[t] = 0.f;
    inv[t] = 1.f;
    if (t < a.T && a.softmax && row) {
      const int n = a.off[t + 1] - a.off[t];
      const float* zt = a.z[t] + b * n;
      float mx = zt[0];
      for (int j = 1; j < n; ++j) mx = fmaxf(mx, zt[j]);
      float sum = 0.f;
      for (int j = 0; j < n; ++j) sum += __expf(zt[j] - mx);
      m[t] = mx;
      inv[t] = 1.f / sum;
    }
  }

  float4 acc[kMixMaxT][NC];
#pragma unroll
  for (int t = 0; t < kMixMaxT; ++t)
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[t][c] = make_float4(0.f, 0.f, 0.f, 0.f);

  for (int e = 0; e < a.E; ++e) {
    const float* xe = a.x[e] + b * a.xs[e];
    const unsigned long long pk = a.pos[e];
    float4 x[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c)
      x[c] = ok[c] ? *reinterpret_cast<const float4*>(xe + 4 * (lig + 64 * c)) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int t = 0; t < kMixMaxT; ++t) {
      if (t < a.T) {
        const int pos = mix_pos(pk, t);
        if (pos != 0xFF) {
          float w = 0.f;
          if (row) {
            const int n = a.off[t + 1] - a.off[t];
            const float zv = a.z[t][b * n + pos];
            w = a.softmax ? __expf(zv - m[t]) * inv[t] : zv;
            if (a.softmax && lig == 0) a.p[b * a.off[a.T] + a.off[t] + pos] = w;
          }
#pragma unroll
          for (int c = 0; c < NC; ++c) {
            acc[t][c].x = fmaf(w, x[c].x, acc[t][c].x);
            acc[t][c].y = fmaf(w, x[c].y, acc[t][c].y);
            acc[t][c].z = fmaf(w, x[c].z, acc[t][c].z);
            acc[t][c].w = fmaf(w, x[c].w, acc[t][c].w);
          }
        }
      }
    }
  }

#pragma unroll
  for (int t = 0; t < kMixMaxT; ++t) {
    if (t < a.T) {
      float* o = a.out + (static_cast<long long>(t) * a.B + b) * (4LL * a.H4);
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (ok[c]) *reinterpret_cast<float4*>(o + 4 * (lig + 64 * c)) = acc[t][c];
    }
  }
}

template <int G, int NC>
__global__ __launch_bounds__(kMixBlock) void mix_bwd_kernel(const MixArgs a) {
  static_assert(NC == 1 || G == 64, "several columns per lane only with whole-wave groups");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lig = lane & (G - 1);
  const long long b = (static_cast<long long>(blockIdx.x) * (kMixBlock / 64) + wave) * (64 / G) + lane / G;
  const bool row = b < a.B;
  const long long H = 4LL * a.H4;
  const int ptot = a.off[a.T];
  bool ok[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) ok[c] = row && lig + 64 * c < a.H4;

  float4 g[kMixMaxT][NC];
  float s[kMixMaxT];
#pragma unroll
  for (int t = 0; t < kMixMaxT; ++t) {
    s[t] = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      g[t][c] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (t < a.T && a.g[t] != nullptr && ok[c]) g[t][c] = *reinterpret_cast<const float4*>(a.g[t] + b * H + 4 * (lig + 64 * c));
    }
  }

  for (int e = 0; e < a.E; ++e) {
    const float* xe = a.x[e] + b * a.xs[e];
    const unsigned long long pk = a.pos[e];
    float4 x[NC], dx[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      x[c] = ok[c] ? *reinterpret_cast<const float4*>(xe + 4 * (lig + 64 * c)) : make_float4(0.f, 0.f, 0.f, 0.f);
      dx[c] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int t = 0; t < kMixMaxT; ++t) {
      if (t < a.T) {
        const int pos = mix_pos(pk, t);
        if (pos != 0xFF && a.g[t] != nullptr) {
          const int n = a.off[t + 1] - a.off[t];
          float w = 0.f;
          if (row) w = a.softmax ? a.p[b * ptot + a.off[t] + pos] : a.z[t][b * n + pos];
#pragma unroll
          for (int c = 0; c < NC; ++c) {
            dx[c].x = fmaf(w, g[t][c].x, dx[c].x);
            dx[c].y = fmaf(w, g[t][c].y, dx[c].y);
            dx[c].z = fmaf(w, g[t][c].z, dx[c].z);
            dx[c].w = fmaf(w, g[t][c].w, dx[c].w);
          }
          if (a.dz[t] != nullptr) {
            float dot = 0.f;
#pragma unroll
            for (int c = 0; c < NC; ++c)
              dot += (x[c].x * g[t][c].x + x[c].y * g[t][c].y) + (x[c].z * g[t][c].z + x[c].w * g[t][c].w);
            dot = group_sum<G>(dot);
            s[t] = fmaf(w, dot, s[t]);
            if (row && lig == (pos & (G - 1))) a.dz[t][b * n + pos] = dot;
          }
        }
      }
    }
    if (a.dx[e] != nullptr) {
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (ok[c]) *reinterpret_cast<float4*>(a.dx[e] + b * H + 4 * (lig + 64 * c)) = dx[c];
    }
  }

  // the lane that parked dp_t[b, j] (lane j mod G of the group) finishes its own entries
#pragma unroll
  for (int t = 0; t < kMixMaxT; ++t) {
    if (t < a.T && a.dz[t] != nullptr && row) {
      const int n = a.off[t + 1] - a.off[t];
      float* dzt = a.dz[t] + b * n;
      if (a.g[t] == nullptr) {
        for (int j = lig; j < n; j += G) dzt[j] = 0.f;
      } else if (a.softmax) {
        const float* pt = a.p + b * ptot + a.off[t];
        for (int j = lig; j < n; j += G) dzt[j] = pt[j] * (dzt[j] - s[t]);
      }
    }
  }
}

// Validates the shape and the selections and fills everything of MixArgs that does not depend on the pass.
static int mix_pack(const char* what, const float* const* x, const int64_t* x_stride, const float* const* z, const int32_t* sel,
                    const int32_t* sel_off, int64_t batch, int32_t hidden, int32_t experts, int32_t gates, int32_t softmax,
                    int32_t dtype, MixArgs* a) {
  if (batch < 0) return fail(RBX_ERR_INVALID, "%s: batch=%lld", what, static_cast<long long>(batch));
  if (!rbx_expert_mix_supported(hidden, experts, gates, sel, sel_off, dtype))
    return fail(RBX_ERR_UNSUPPORTED,
                "%s: needs float32, hidden=%d a multiple of 4 in [%d,%d], experts=%d in [1,%d], gates=%d in [1,%d] and per gate "
                "1..%d distinct experts", what, hidden, kMixMinH, kMixMaxH, experts, kMixMaxE, gates, kMixMaxT, kMixMaxN);
  if (batch == 0) return RBX_OK;
  if (!x || !x_stride || !z) return fail(RBX_ERR_INVALID, "%s: NULL pointer array", what);
  *a = MixArgs{};
  for (int e = 0; e < experts; ++e) {
    if (!x[e]) return fail(RBX_ERR_INVALID, "%s: expert %d is NULL", what, e);
    if (!aligned16(x[e]) || (x_stride[e] & 3) != 0 || x_stride[e] < 0)
      return fail(RBX_ERR_UNSUPPORTED, "%s: expert %d must be 16-byte aligned with a row stride that is a multiple of 4 floats",
                  what, e);
    a->x[e] = x[e];
    a->xs[e] = x_stride[e];
    a->pos[e] = ~0ULL;
  }
  for (int t = 0; t < gates; ++t) {
    if (!z[t]) return fail(RBX_ERR_INVALID, "%s: gate %d is NULL", what, t);
    a->z[t] = z[t];
    a->off[t] = sel_off[t];
    for (int j = sel_off[t]; j < sel_off[t + 1]; ++j) {
      unsigned long long& pk = a->pos[sel[j]];
      pk = (pk & ~(0xFFULL << (8 * t))) | (static_cast<unsigned long long>(j - sel_off[t]) << (8 * t));
    }
  }
  a->off[gates] = sel_off[gates];
  a->B = batch;
  a->H4 = hidden / 4;
  a->E = experts;
  a->T = gates;
  a->softmax = softmax != 0;
  const int group = a->H4 >= 64 ? 64 : pow2_ceil(a->H4);
  for (a->lg = 0; (1 << a->lg) < group; ++a->lg) {}
  const long long per_block = (kMixBlock / 64) * (64 >> a->lg);
  if ((batch + per_block - 1) / per_block > INT_MAX)
    return fail(RBX_ERR_UNSUPPORTED, "%s: batch=%lld is too large", what, static_cast<long long>(batch));
  return RBX_OK;
}

static dim3 mix_grid(const MixArgs& a) {
  const long long per_block = (kMixBlock / 64) * (64 >> a.lg);
  return dim3(static_cast<unsigned>((a.B + per_block - 1) / per_block));
}

}  // namespace rbx

extern "C" int rbx_expert_mix_supported(int32_t hidden, int32_t experts, int32_t gates, const int32_t* sel,
                                        const int32_t* sel_off, int32_t dtype) {
  using namespace rbx;
  if (dtype != RBX_F32 || hidden < kMixMinH || hidden > kMixMaxH || (hidden & 3) != 0) return 0;
  if (experts < 1 || experts > kMixMaxE || gates < 1 || gates > kMixMaxT || !sel || !sel_off || sel_off[0] != 0) return 0;
  for (int t = 0; t < gates; ++t) {
    const int n = sel_off[t + 1] - sel_off[t];
    if (n < 1 || n > kMixMaxN) return 0;
    unsigned seen = 0;
    for (int j = sel_off[t]; j < sel_off[t + 1]; ++j) {
      if (sel[j] < 0 || sel[j] >= experts || (seen >> sel[j]) & 1u) return 0;
      seen |= 1u << sel[j];
    }
  }
  return 1;
}

extern "C" int rbx_expert_mix_fwd(const float* const* x, const int64_t* x_stride, const float* const* z, const int32_t* sel,
                                  const int32_t* sel_off, int64_t batch, int32_t hidden, int32_t experts, int32_t gates,
                                  int32_t softmax, int32_t dtype, float* d_out, float* d_p, void* stream) {
  using namespace rbx;
  MixArgs a;
  const int rc = mix_pack("expert_mix_fwd", x, x_stride, z, sel, sel_off, batch, hidden, experts, gates, softmax, dtype, &a);
  if (rc != RBX_OK || batch == 0) return rc;
  if (!d_out || (softmax && !d_p)) return fail(RBX_ERR_INVALID, "expert_mix_fwd: NULL output");
  if (!aligned16(d_out)) return fail(RBX_ERR_UNSUPPORTED, "expert_mix_fwd: out must be 16-byte aligned");
  a.out = d_out;
  a.p = d_p;
  const dim3 grid = mix_grid(a), block(kMixBlock);
  hipStream_t s = as_stream(stream);
  switch ((a.H4 + 63) / 64) {
    case 1: hipLaunchKernelGGL(mix_fwd_kernel<1>, grid, block, 0, s, a); break;
    case 2: hipLaunchKernelGGL(mix_fwd_kernel<2>, grid, block, 0, s, a); break;
    case 3: hipLaunchKernelGGL(mix_fwd_kernel<3>, grid, block, 0, s, a); break;
    default: hipLaunchKernelGGL(mix_fwd_kernel<4>, grid, block, 0, s, a); break;
  }
  return check_launch("expert_mix_fwd");
}

extern "C" int rbx_expert_mix_bwd(const float* const* x, const int64_t* x_stride, const float* const* z, const float* d_p,
                                  const float* const* dout, const int32_t* sel, const int32_t* sel_off, int64_t batch,
                                  int32_t hidden, int32_t experts, int32_t gates, int32_t softmax, int32_t dtype,
                                  float* const* dx, float* const* dz, void* stream) {
  using namespace rbx;
  MixArgs a;
  const int rc = mix_pack("expert_mix_bwd", x, x_stride, z, sel, sel_off, batch, hidden, experts, gates, softmax, dtype, &a);
  if (rc != RBX_OK || batch == 0) return rc;
  if (!dout || (softmax && !d_p)) return fail(RBX_ERR_INVALID, "expert_mix_bwd: NULL pointer array");
  for (int t = 0; t < gates; ++t) {
    if (dout[t] != nullptr && !aligned16(dout[t]))
      return fail(RBX_ERR_UNSUPPORTED, "expert_mix_bwd: dout %d must be 16-byte aligned", t);
    a.g[t] = dout[t];
    a.dz[t] = dz ? dz[t] : nullptr;
  }
  for (int e = 0; e < experts; ++e) {
    a.dx[e] = dx ? dx[e] : nullptr;
    if (a.dx[e] != nullptr && !aligned16(a.dx[e]))
      return fail(RBX_ERR_UNSUPPORTED, "expert_mix_bwd: dx %d must be 16-byte aligned", e);
  }
  a.p = const_cast<float*>(d_p);
  const dim3 grid = mix_grid(a), block(kMixBlock);
  hipStream_t s = as_stream(stream);
#define RBX_MIX_BWD(G, NC) hipLaunchKernelGGL((mix_bwd_kernel<G, NC>), grid, block, 0, s, a)
  switch ((a.H4 + 63) / 64) {
    case 1:
      switch (a.lg) {
        case 0: RBX_MIX_BWD(1, 1); break;
        case 1: RBX_MIX_BWD(2, 1); break;
        case 2: RBX_MIX_BWD(4, 1); break;
        case 3: RBX_MIX_BWD(8, 1); break;
        case 4: RBX_MIX_BWD(16, 1); break;
        case 5: RBX_MIX_BWD(32, 1); break;
        default: RBX_MIX_BWD(64, 1); break;
      }
      break;
    case 2: RBX_MIX_BWD(64, 2); break;
    case 3: RBX_MIX_BWD(64, 3); break;
    default: RBX_MIX_BWD(64, 4); break;
  }
#undef RBX_MIX_BWD
  return check_launch("expert_mix_bwd");
}
