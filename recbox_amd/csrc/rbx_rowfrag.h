// rbx_rowfrag.h -- a lane's register share of an embedding row in the gather kernels (rbx_embed_fwd.hip: padded ids;
// rbx_embed_csr.hip: ragged bags).  Both kernels sum rows through these operations, in the same order.
#pragma once
#include "rbx_internal.h"

namespace rbx {

// The shape of the pooled gather, shared by embed_seq_kernel and bag_walk_kernel: the two are bit-equal on the same live
// ids because chunks (G * kSeqIpl ids), row batches and sub-group counts are the same numbers, defined once.
constexpr int kSeqWaves = 4;           // waves per SIMD the kernels are bounded for
constexpr int kSeqU = 4;               // rows in flight per lane
constexpr int kSeqIpl = 4;             // ids per lane per chunk (chunk = 64 .. 256 lookups)
// lanes of the group that pools one (sample, sequence feature) or one bag, for rows of G lanes: narrow rows share a
// wider group as R = seq_group_lanes(G) / G sub-groups
constexpr int seq_group_lanes(int G) { return (G <= 8) ? 16 : ((G == 16) ? 32 : 64); }

template <bool VEC>
struct Acc;
template <>
struct Acc<true> {
  float4 v;
  __device__ __forceinline__ void zero() { v = make_float4(0.f, 0.f, 0.f, 0.f); }
  __device__ __forceinline__ void add(const Acc& o) { v.x += o.v.x; v.y += o.v.y; v.z += o.v.z; v.w += o.v.w; }
  __device__ __forceinline__ void scale(float s) { v.x *= s; v.y *= s; v.z *= s; v.w *= s; }
  __device__ __forceinline__ float hsum() const { return (v.x + v.y) + (v.z + v.w); }
  __device__ __forceinline__ void load(const float* p) { v = *reinterpret_cast<const float4*>(p); }
  __device__ __forceinline__ void store(float* p) const { *reinterpret_cast<float4*>(p) = v; }
  __device__ __forceinline__ void xor_add(int o) {
    v.x += __shfl_xor(v.x, o, 64); v.y += __shfl_xor(v.y, o, 64);
    v.z += __shfl_xor(v.z, o, 64); v.w += __shfl_xor(v.w, o, 64);
  }
  __device__ __forceinline__ float& at(int k) { return k == 0 ? v.x : (k == 1 ? v.y : (k == 2 ? v.z : v.w)); }
  __device__ __forceinline__ Acc xor_get(int o) const {
    Acc r;
    r.v = make_float4(__shfl_xor(v.x, o, 64), __shfl_xor(v.y, o, 64), __shfl_xor(v.z, o, 64), __shfl_xor(v.w, o, 64));
    return r;
  }
};
template <>
struct Acc<false> {
  float v;
  __device__ __forceinline__ void zero() { v = 0.f; }
  __device__ __forceinline__ void add(const Acc& o) { v += o.v; }
  __device__ __forceinline__ void scale(float s) { v *= s; }
  __device__ __forceinline__ float hsum() const { return v; }
  __device__ __forceinline__ void load(const float* p) { v = *p; }
  __device__ __forceinline__ void store(float* p) const { *p = v; }
  __device__ __forceinline__ void xor_add(int o) { v += __shfl_xor(v, o, 64); }
  __device__ __forceinline__ float& at(int) { return v; }
  __device__ __forceinline__ Acc xor_get(int o) const {
    Acc r;
    r.v = __shfl_xor(v, o, 64);
    return r;
  }
};

// One lane's share of a row: NV units, unit u covers elements [(lane_g + u*G)*W, +W).
template <int G, int NV, bool VEC>
struct RowFrag {
  static constexpr int W = VEC ? 4 : 1;
  Acc<VEC> a[NV];
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int u = 0; u < NV; ++u) a[u].zero();
  }
  __device__ __forceinline__ void load(const float* row, int dim, int lane_g) {
#pragma unroll
    for (int u = 0; u < NV; ++u) {
      const int e = (lane_g + u * G) * W;
      if (e < dim) a[u].load(row + e); else a[u].zero();
    }
  }
  __device__ __forceinline__ void store(float* row, int dim, int lane_g) const {
#pragma unroll
    for (int u = 0; u < NV; ++u) {
      const int e = (lane_g + u * G) * W;
      if (e < dim) a[u].store(row + e);
    }
  }
  __device__ __forceinline__ void add(const RowFrag& o) {
#pragma unroll
    for (int u = 0; u < NV; ++u) a[u].add(o.a[u]);
  }
  __device__ __forceinline__ void scale(float s) {
#pragma unroll
    for (int u = 0; u < NV; ++u) a[u].scale(s);
  }
  __device__ __forceinline__ float hsum() const {
    float s = 0.f;
#pragma unroll
    for (int u = 0; u < NV; ++u) s += a[u].hsum();
    return s;
  }
  __device__ __forceinline__ void xor_add(int o) {
#pragma unroll
    for (int u = 0; u < NV; ++u) a[u].xor_add(o);
  }
  // For an op that selects instead of adding (the max pool): the share element by element, q = u * W + k, and the share
  // of lane ^ o.  With q a constant of an unrolled loop `at` is a register name.
  static constexpr int kElems = NV * W;
  __device__ __forceinline__ float& at(int q) { return a[q / W].at(q % W); }
  __device__ __forceinline__ RowFrag xor_get(int o) const {
    RowFrag r;
#pragma unroll
    for (int u = 0; u < NV; ++u) r.a[u] = a[u].xor_get(o);
    return r;
  }
};

}  // namespace rbx
