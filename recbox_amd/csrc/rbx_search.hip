// rbx_search.hip -- SURVEY 8f-2: IndexFlatIP.search as ONE fused op (gfx950): the k items with the largest inner
// product per user, without the [users, n_items] score matrix.
//
// Reference behaviour replaced: FaissIndex(IndexFlatIP).search(user_embs, topk=500), utils/ann/faiss.py:3-15 as used by
// core/metrics.py:56.  rbx_linear_fwd + rbx_topk serve it by writing scores = U I^T to HBM and reading them back; at
// 10 M items that matrix limits a block to 26 users and every block re-reads the item table.  rbx_topk's fast path for
// long rows (threshold from 8 192 strided samples, one filtering sweep, exact selection among <= 8 192 candidates, a
// per-row flag for rows the estimate cannot serve) reads every score exactly once, to compare it: here that comparison
// is the GEMM's epilogue, on the accumulator registers.
//
// search_ip_kernel: U-stationary fp32 score kernel on v_mfma_f32_32x32x2_f32 (exact fp32 products and accumulation,
// like gemm_f32_kernel).  A 256-thread workgroup keeps 64 user rows [64, dim] k-major in LDS for its whole life and walks
// a contiguous range of 128-item tiles through a double-buffered LDS ring of [16 k, 128 items] slices; a wavefront owns
// 64 users x 32 items (two 32 x 32 accumulators).  Items are read at a row stride `item_ld`, so the sampling pass is the
// same kernel over 8 192 "items" at item_ld = stride * dim: no gather, no copy.  Epilogues:
//   store   out[row, col] = score                                       (the sample [rows, 8 192])
//   filter  key_of(score) >= thr[row]: (score, item) -> an LDS stage; a flush hands the stage to the rows' candidate
//           slots with one atomicAdd(&cnt[row], mine) per (workgroup, row).  A stage that is full or a row whose
//           kTopkCand slots are used up sets fail[row] (the row is then served by the caller's matrix path).
// Candidate order depends on the atomics; the final topk_kernel selects by (key, item), so the result does not.
#include "rbx_topk.h"

namespace rbx {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kSearchBM = 64, kSearchBN = 128, kSearchBK = 16;
constexpr int kSearchLdu = kSearchBM + 4;      // LDS pitch of a k row of the user tile (floats)
constexpr int kSearchLdi = kSearchBN + 4;      // ... of the item ring
constexpr int kSearchMaxDim = 512;
constexpr int kSearchXcds = 8;
constexpr int kSearchStageMin = 512, kSearchStageMax = 4096;
constexpr size_t kSearchLdsMax = 163840 - 1024;   // 160 KiB per workgroup less the kernel's static words
constexpr unsigned kNoBase = 0xFFFFFFFFu;

// One [128 items, 16 k] slice of the item operand, global -> registers: thread t takes k = 4 (t % 4) .. + 3 of items
// t / 4 and t / 4 + 64.  Items beyond n and k beyond dim read as zero.
__device__ __forceinline__ void search_load_items(const float* __restrict__ I, const long long item_ld, const long long n0,
                                                  const int k0, const int n, const int dim, const bool vec,
                                                  float (&reg)[8]) {
  const int t = threadIdx.x;
  const int k = k0 + (t & 3) * 4;
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const long long item = n0 + (t >> 2) + 64 * p;
    const float* src = I + item * item_ld + k;
    if (item < n && k + 3 < dim) {
      if (vec) {
        const float4 v = *reinterpret_cast<const float4*>(src);
        reg[p * 4 + 0] = v.x; reg[p * 4 + 1] = v.y; reg[p * 4 + 2] = v.z; reg[p * 4 + 3] = v.w;
      } else {                                      // rows that are not 16-byte aligned: four plain loads
        reg[p * 4 + 0] = src[0]; reg[p * 4 + 1] = src[1]; reg[p * 4 + 2] = src[2]; reg[p * 4 + 3] = src[3];
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) reg[p * 4 + j] = (item < n && k + j < dim) ? src[j] : 0.f;
    }
  }
}
__device__ __forceinline__ void search_store_items(float* __restrict__ tile, const float (&reg)[8]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int j = 0; j < 4; ++j) tile[((t & 3) * 4 + j) * kSearchLdi + (t >> 2) + 64 * p] = reg[p * 4 + j];
}

// Dynamic LDS: user tile [dimp][68] | item ring 2 x [16][132] | stage: score[cap], item[cap], (row << 16 | rank)[cap]
template <bool FILTER>
__global__ __launch_bounds__(256) void search_ip_kernel(const float* __restrict__ U, const long long user_stride,
                                                        const long long rows, const float* __restrict__ I,
                                                        const long long item_ld, const int n, const int dim, const int dimp,
                                                        const int ranges, const int tiles_per_range, const int n_tiles,
                                                        const int total, const bool vec_i, float* __restrict__ out,
                                                        const long long ldo, const unsigned* __restrict__ thr,
                                                        unsigned* __restrict__ cnt, unsigned* __restrict__ fail,
                                                        float* __restrict__ cand_vals, long long* __restrict__ cand_pos,
                                                        const int stage_cap) {
  extern __shared__ float smem[];
  __shared__ unsigned s_thr[kSearchBM], s_cnt[kSearchBM], s_base[kSearchBM];
  __shared__ unsigned s_n;
  float* Us = smem;
  float* Is = Us + dimp * kSearchLdu;
  float* st_val = Is + 2 * kSearchBK * kSearchLdi;
  unsigned* st_item = reinterpret_cast<unsigned*>(st_val + stage_cap);
  unsigned* st_meta = st_item + stage_cap;

  // Workgroups that share a user tile on one XCD (launch index L runs on XCD L % 8; XCD x works through one contiguous
  // range of the (user tile, item range) pairs, item range fastest): the arithmetic of gemm_f32_kernel.
  int ut, rg;
  {
    const int L = static_cast<int>(blockIdx.x);
    const int xcd = L % kSearchXcds, slot = L / kSearchXcds;
    const int q = total / kSearchXcds, rem = total % kSearchXcds;
    const int work = xcd * q + (xcd < rem ? xcd : rem) + slot;
    ut = work / ranges;
    rg = work % ranges;
  }
  const int t_begin = rg * tiles_per_range;
  const int t_end = (t_begin + tiles_per_range < n_tiles) ? t_begin + tiles_per_range : n_tiles;
  if (t_begin >= t_end) return;
  const long long m0 = static_cast<long long>(ut) * kSearchBM;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wn = (tid >> 6) * 32;
  const int li = lane & 31, lk = lane >> 5;

  // the user tile, once: k-major, rows beyond `rows` and k beyond dim are zero
  for (int e = tid; e < kSearchBM * dimp; e += 256) {
    const int m = e / dimp, k = e - m * dimp;
    Us[k * kSearchLdu + m] = (m0 + m < rows && k < dim) ? U[(m0 + m) * user_stride + k] : 0.f;
  }
  if (FILTER && tid < kSearchBM) {
    s_thr[tid] = (m0 + tid < rows) ? thr[m0 + tid] : 0xFFFFFFFFu;
    s_cnt[tid] = 0u;
  }
  if (tid == 0) s_n = 0u;

  // hand the stage to the rows' candidate slots; every thread of the workgroup calls it
  auto flush = [&]() {
    __syncthreads();
    const unsigned staged = s_n < static_cast<unsigned>(stage_cap) ? s_n : static_cast<unsigned>(stage_cap);
    if (tid < kSearchBM) {
      const unsigned mine = s_cnt[tid];
      unsigned base = kNoBase;
      if (mine > 0u) {
        base = atomicAdd(&cnt[m0 + tid], mine);
        if (base + mine > static_cast<unsigned>(kTopkCand)) {
          atomicOr(&fail[m0 + tid], 1u);
          base = kNoBase;
        }
      }
      s_base[tid] = base;
      s_cnt[tid] = 0u;
    }
    __syncthreads();
    for (unsigned j = tid; j < staged; j += 256) {
      const unsigned meta = st_meta[j];
      const unsigned r = meta >> 16, base = s_base[r];
      if (base == kNoBase) continue;
      const long long slot = (m0 + r) * kTopkCand + base + (meta & 0xFFFFu);
      cand_vals[slot] = st_val[j];
      cand_pos[slot] = static_cast<long long>(st_item[j]);
    }
    __syncthreads();
    if (tid == 0) s_n = 0u;
    __syncthreads();
  };

  const int ksteps = dimp / kSearchBK;
  float reg[8];
  search_load_items(I, item_ld, static_cast<long long>(t_begin) * kSearchBN, 0, n, dim, vec_i, reg);
  search_store_items(Is, reg);
  __syncthreads();
  int cur = 0;
  for (int tile = t_begin; tile < t_end; ++tile) {
    const long long n0 = static_cast<long long>(tile) * kSearchBN;
    f32x16 acc[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
    for (int ks = 0; ks < ksteps; ++ks) {
      const bool last_k = ks + 1 == ksteps;
      const int nt = last_k ? tile + 1 : tile, nk = last_k ? 0 : (ks + 1) * kSearchBK;
      const bool more = nt < t_end;
      if (more) search_load_items(I, item_ld, static_cast<long long>(nt) * kSearchBN, nk, n, dim, vec_i, reg);   // flies under the MFMAs
      const float* us = Us + ks * kSearchBK * kSearchLdu;
      const float* is = Is + cur * kSearchBK * kSearchLdi;
#pragma unroll
      for (int kk = 0; kk < kSearchBK; kk += 2) {
        const float a0 = us[(kk + lk) * kSearchLdu + li];
        const float a1 = us[(kk + lk) * kSearchLdu + 32 + li];
        const float b = is[(kk + lk) * kSearchLdi + wn + li];
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b, acc[1], 0, 0, 0);
      }
      if (more) search_store_items(Is + (cur ^ 1) * kSearchBK * kSearchLdi, reg);
      __syncthreads();
      cur ^= 1;
    }
    // epilogue; C/D layout of the 32 x 32 MFMA: col = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
    const long long col = n0 + wn + li;
    if constexpr (!FILTER) {
      if (col < n) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const long long row = m0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
            if (row < rows) out[row * ldo + col] = acc[i][r];
          }
      }
    } else {
      if (col < n) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int rl = i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
            const float v = acc[i][r];
            if (m0 + rl < rows && key_of(v) >= s_thr[rl]) {
              const unsigned slot = atomicAdd(&s_n, 1u);
              if (slot < static_cast<unsigned>(stage_cap)) {
                const unsigned rank = atomicAdd(&s_cnt[rl], 1u);
                st_val[slot] = v;
                st_item[slot] = static_cast<unsigned>(col);
                st_meta[slot] = (static_cast<unsigned>(rl) << 16) | rank;
              } else {
                atomicOr(&fail[m0 + rl], 1u);       // the stage is full: this row lost a candidate
              }
            }
          }
      }
      // flush when the stage is half full (the host sizes it for two tiles' expected survivors and a margin), and at the end
      __syncthreads();
      if (2u * s_n > static_cast<unsigned>(stage_cap) || tile + 1 == t_end) flush();
    }
  }
}

struct SearchPlan {
  long long m, sstride;
  int rank, dimp, stage_cap;
  size_t lds_store, lds_filter;
};

// false: the fused search does not serve this shape
static bool search_plan(long long rows, long long n_items, int dim, int k, SearchPlan* p) {
  if (rows <= 0 || n_items <= 0 || k <= 0 || k > kTopkMaxK || dim < 1 || dim > kSearchMaxDim) return false;
  if (n_items >= (1ll << 31)) return false;
  if ((rows + kSearchBM - 1) / kSearchBM >= (1 << 20)) return false;
  p->rank = topk_sample_rank(n_items, k, &p->m, &p->sstride);
  if (p->rank <= 0) return false;
  // rbx_topk's rank carries a margin of 8 sample ranks, i.e. 8 n / 8192 expected candidates: beyond ~4 M items that alone
  // overflows the 8 192 slots (measured at 10 M items, k = 500: 848 of 1000 rows not served).  Here the rank is capped so that
  // kTopkCand / 2 candidates are expected -- but never below twice the rank that k itself asks for, plus 2.
  {
    const long long hi = (kTopkCand / 2) / p->sstride, lo = (2ll * k + p->sstride - 1) / p->sstride + 2;
    const long long cap = hi > lo ? hi : lo;
    if (p->rank > cap) p->rank = static_cast<int>(cap);
  }
  p->dimp = (dim + kSearchBK - 1) / kSearchBK * kSearchBK;
  const size_t fixed = (static_cast<size_t>(p->dimp) * kSearchLdu + 2 * kSearchBK * kSearchLdi) * sizeof(float);
  // a tile holds 64 x 128 = 8 192 scores, of which rank in 8 192 are expected above the threshold
  int cap = pow2_ceil(2 * p->rank + 256);
  cap = cap < kSearchStageMin ? kSearchStageMin : (cap > kSearchStageMax ? kSearchStageMax : cap);
  while (cap > kSearchStageMin && fixed + static_cast<size_t>(cap) * 12 > kSearchLdsMax) cap >>= 1;
  p->stage_cap = cap;
  p->lds_store = fixed;
  p->lds_filter = fixed + static_cast<size_t>(cap) * 12;
  return p->lds_filter <= kSearchLdsMax;
}

static size_t search_head_bytes(long long rows) { return (static_cast<size_t>(rows) * 3 * sizeof(unsigned) + 255) / 256 * 256; }

template <bool FILTER>
static int search_launch(const float* U, long long user_stride, long long rows, const float* I, long long item_ld, int n,
                         int dim, const SearchPlan& p, size_t lds, float* out, long long ldo, const unsigned* thr,
                         unsigned* cnt, unsigned* failed, float* cval, long long* cpos, hipStream_t s) {
  const int tiles_u = static_cast<int>((rows + kSearchBM - 1) / kSearchBM);
  const int n_tiles = (n + kSearchBN - 1) / kSearchBN;
  // enough item ranges that one user tile still fills the chip, not more workgroups than are resident at once
  int occ = static_cast<int>((kSearchLdsMax + 1024) / (lds + 1024));
  occ = occ < 1 ? 1 : (occ > 4 ? 4 : occ);
  int ranges = (kCUs * occ) / tiles_u;
  ranges = ranges < 1 ? 1 : (ranges > n_tiles ? n_tiles : ranges);
  const int tpr = (n_tiles + ranges - 1) / ranges;
  ranges = (n_tiles + tpr - 1) / tpr;
  const long long total = static_cast<long long>(tiles_u) * ranges;
  if (total >= INT_MAX) return fail(RBX_ERR_UNSUPPORTED, "search_ip: too many rows");
  const bool vec = (reinterpret_cast<uintptr_t>(I) & 15) == 0 && (item_ld & 3) == 0;
  const int lrc = allow_lds("search_ip", &search_ip_kernel<FILTER>, lds);
  if (lrc != RBX_OK) return lrc;
  hipLaunchKernelGGL((search_ip_kernel<FILTER>), dim3(static_cast<unsigned>(total)), dim3(256), lds, s, U, user_stride, rows,
                     I, item_ld, n, dim, p.dimp, ranges, tpr, n_tiles, static_cast<int>(total), vec, out, ldo, thr, cnt,
                     failed, cval, cpos, FILTER ? p.stage_cap : 0);
  return RBX_OK;
}

}  // namespace rbx

extern "C" size_t rbx_search_ip_workspace_size(int64_t rows, int64_t n_items, int32_t dim, int32_t k) {
  rbx::SearchPlan p;
  if (!rbx::search_plan(rows, n_items, dim, k, &p)) return 0;
  // thr, cnt, fail | candidate items [rows, 8192] int64 | candidate scores [rows, 8192] (first the sample's scores)
  return rbx::search_head_bytes(rows) + static_cast<size_t>(rows) * rbx::kTopkCand * (sizeof(int64_t) + sizeof(float));
}

extern "C" int rbx_search_ip(const float* d_users, int64_t rows, int64_t user_stride, const float* d_items, int64_t n_items,
                             int32_t dim, int32_t k, float* d_out_scores, int64_t* d_out_index, int32_t* d_row_state,
                             void* d_workspace, size_t workspace_bytes, void* stream) {
  using namespace rbx;
  if (rows < 0 || n_items < 0) return fail(RBX_ERR_INVALID, "search_ip: negative sizes");
  if (rows == 0) return RBX_OK;
  if (dim < 1 || dim > kSearchMaxDim) return fail(RBX_ERR_UNSUPPORTED, "search_ip: dim=%d not in [1,%d]", dim, kSearchMaxDim);
  if (k <= 0 || k > kTopkMaxK) return fail(RBX_ERR_UNSUPPORTED, "search_ip: k=%d not in [1,%d]", k, kTopkMaxK);
  if (n_items >= (1ll << 31)) return fail(RBX_ERR_UNSUPPORTED, "search_ip: 2^31 items or more are not supported");
  SearchPlan p;
  if (!search_plan(rows, n_items, dim, k, &p))
    return fail(RBX_ERR_UNSUPPORTED, "search_ip: n_items=%lld, k=%d is not selective enough for the sampled threshold "
                "(use rbx_linear_fwd + rbx_topk)", static_cast<long long>(n_items), k);
  if (!d_users || !d_items || !d_out_scores || !d_out_index || !d_row_state)
    return fail(RBX_ERR_INVALID, "search_ip: NULL tensor");
  if (user_stride < dim) return fail(RBX_ERR_INVALID, "search_ip: user_stride < dim");
  if (d_workspace == nullptr || workspace_bytes < rbx_search_ip_workspace_size(rows, n_items, dim, k))
    return fail(RBX_ERR_WORKSPACE, "search_ip: workspace too small");
  hipStream_t s = as_stream(stream);
  unsigned* thr = static_cast<unsigned*>(d_workspace);
  unsigned* cnt = thr + rows;
  unsigned* failed = cnt + rows;
  long long* cpos = reinterpret_cast<long long*>(static_cast<char*>(d_workspace) + search_head_bytes(rows));
  float* cval = reinterpret_cast<float*>(cpos + rows * kTopkCand);
  float* sample = cval;                      // read by (2), before (4) writes candidates over it
  // (1) scores of the 8 192 sampled items (item j * sstride): the same kernel at a row stride of sstride * dim
  int rc = search_launch<false>(d_users, user_stride, rows, d_items, p.sstride * dim, static_cast<int>(p.m), dim, p,
                                p.lds_store, sample, static_cast<long long>(kTopkCand), nullptr, nullptr, nullptr, nullptr,
                                nullptr, s);
  if (rc != RBX_OK) return rc;
  // (2) threshold = key of the rank-th largest sample
  topk_launch_threshold(sample, rows, static_cast<long long>(kTopkCand), p.m, 1ll, p.rank, thr, s);
  // (3)
  if (hipMemsetAsync(cnt, 0, static_cast<size_t>(rows) * 2 * sizeof(unsigned), s) != hipSuccess)
    return fail(RBX_ERR_LAUNCH, "search_ip: memset of the candidate counters failed");
  // (4) the sweep over all items keeps what is >= threshold; no score reaches HBM
  rc = search_launch<true>(d_users, user_stride, rows, d_items, static_cast<long long>(dim), static_cast<int>(n_items), dim, p,
                           p.lds_filter, nullptr, 0ll, thr, cnt, failed, cval, cpos, s);
  if (rc != RBX_OK) return rc;
  // (5) which rows have what they need, (6) exact selection + sort among their candidates
  topk_launch_state(cnt, failed, rows, static_cast<unsigned>(k), d_row_state, s);
  topk_launch_candidates(cval, cpos, cnt, d_row_state, rows, k, d_out_scores, reinterpret_cast<long long*>(d_out_index),
                         nullptr, 0ll, s);
  return check_launch("search_ip");
}
