// rbx_topk.h -- what rbx_topk.hip shares with the fused inner-product search (rbx_search.hip): the key encoding,
// the constants of the sampled-threshold fast path and host-side launchers of its selection kernels.
#pragma once
#include "rbx_internal.h"

namespace rbx {

constexpr int kTopkMaxK = 1024;
constexpr int kTopkSeg = 8192;        // scores per workgroup: their keys are staged in LDS once (32 KB)
constexpr int kTopkCand = kTopkSeg;   // candidate slots per row (one segment of the final selection)

__device__ __forceinline__ unsigned key_of(float v) {
  const unsigned u = __float_as_uint(v);
  // larger float <=> larger key, equal floats <=> equal keys: -0.0 (0x80000000) takes the key of +0.0, so that the two
  // zeros tie and the lower index decides between them (value_of returns +0.0 for either)
  return (u > 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ unsigned long long pack_winner(unsigned key, long long index) {
  return (static_cast<unsigned long long>(key) << 32) | static_cast<unsigned>(~static_cast<unsigned>(index));
}
__device__ __forceinline__ float value_of(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// sample rank for the threshold estimate, or 0 when the fast path does not apply (short rows, k not selective)
inline int topk_sample_rank(long long n, int k, long long* m_out, long long* stride_out) {
  if (n <= 2ll * kTopkSeg) return 0;
  const long long m = kTopkSeg, stride = n / m;
  const long long r = (4ll * k * m + n - 1) / n + 8;
  *m_out = m;
  *stride_out = stride;
  return (r < m / 4) ? static_cast<int>(r) : 0;
}

// The three selection steps of the fast path (defined in rbx_topk.hip; launches only, the caller checks them):
//   thr[u] = key of the rank-th largest of the m samples vals[u * row_stride + j * sample_stride], j < m
void topk_launch_threshold(const float* vals, long long rows, long long row_stride, long long m, long long sample_stride,
                           int rank, unsigned* thr, hipStream_t s);
//   state[u] = 1 when row u has no overflow and between `need` and kTopkCand candidates, else 0
void topk_launch_state(const unsigned* cnt, const unsigned* fail, long long rows, unsigned need, int* state, hipStream_t s);
//   exact top k, sorted, among the cnt[u] candidates (cval, cpos)[u, 0..kTopkCand) of the rows with state[u] == 1;
//   remap (optional): the reported index of row position p is remap[u * remap_stride + p]
void topk_launch_candidates(const float* cval, const long long* cpos, const unsigned* cnt, const int* state, long long rows,
                            int k, float* out_vals, long long* out_idx, const long long* remap, long long remap_stride,
                            hipStream_t s);

}  // namespace rbx
