// rbx_gemm_f32.h -- the tiled GEMM on v_mfma_f32_32x32x2_f32 (exact f32 products): operand staging, the steady k loop with
// its untested loads, the narrow companion for a tail of <= 64 output columns, and gemm_f32_kernel (all three operand
// layouts, split K).  Included by rbx_dense.hip behind rbx_gemm_tile.h.
#pragma once
#include <type_traits>
#include "rbx_gemm_tile.h"

namespace rbx {

// Load one 128 x BK operand tile into registers (BK/2 floats per thread).
//   KCONTIG: element (r, k) at base[r * ld + k]   -> thread reads float4 along k
//   else   : element (r, k) at base[k * ld + r]   -> thread reads float4 along r
constexpr int KT = BK / 4;            // threads along k of a k-contiguous tile
constexpr int NP = BK / 8;            // float4 loads per thread and operand
template <bool KCONTIG>
__device__ __forceinline__ void load_tile(const float* __restrict__ base, long long ld, int r0, int k0, int R, int K,
                                          bool vec_ok, float (&reg)[4 * NP]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    if constexpr (KCONTIG) {
      const int r = r0 + t / KT + (256 / KT) * p;
      const int k = k0 + (t % KT) * 4;
      const float* src = base + static_cast<long long>(r) * ld + k;
      if (vec_ok && r < R && k + 3 < K) {
        const float4 v = *reinterpret_cast<const float4*>(src);
        reg[p * 4 + 0] = v.x; reg[p * 4 + 1] = v.y; reg[p * 4 + 2] = v.z; reg[p * 4 + 3] = v.w;
      } else if (r < R && k + 3 < K) {              // unaligned rows (K = 1677): four plain loads, no per-element tests
        reg[p * 4 + 0] = src[0]; reg[p * 4 + 1] = src[1]; reg[p * 4 + 2] = src[2]; reg[p * 4 + 3] = src[3];
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) reg[p * 4 + j] = (r < R && k + j < K) ? src[j] : 0.f;
      }
    } else {
      const int k = k0 + (t >> 5) + 8 * p;
      const int r = r0 + (t & 31) * 4;
      const float* src = base + static_cast<long long>(k) * ld + r;
      if (vec_ok && k < K && r + 3 < R) {
        const float4 v = *reinterpret_cast<const float4*>(src);
        reg[p * 4 + 0] = v.x; reg[p * 4 + 1] = v.y; reg[p * 4 + 2] = v.z; reg[p * 4 + 3] = v.w;
      } else if (k < K && r + 3 < R) {
        reg[p * 4 + 0] = src[0]; reg[p * 4 + 1] = src[1]; reg[p * 4 + 2] = src[2]; reg[p * 4 + 3] = src[3];
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) reg[p * 4 + j] = (k < K && r + j < R) ? src[j] : 0.f;
      }
    }
  }
}

template <bool KCONTIG>
__device__ __forceinline__ void store_tile(float* __restrict__ tile, const float (&reg)[4 * NP]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    if constexpr (KCONTIG) {
      const int r = t / KT + (256 / KT) * p;
      const int k = (t % KT) * 4;
#pragma unroll
      for (int j = 0; j < 4; ++j) tile[(k + j) * LDT + r] = reg[p * 4 + j];
    } else {
      const int k = (t >> 5) + 8 * p;
      const int r = (t & 31) * 4;
      *reinterpret_cast<float4*>(&tile[k * LDT + r]) = make_float4(reg[p * 4], reg[p * 4 + 1], reg[p * 4 + 2], reg[p * 4 + 3]);
    }
  }
}

// Steady-state loads of a k tile that lies inside [kbeg, kend): per-thread offsets that advance by one k tile per step --
// no tests, no branches, no address arithmetic beyond one 64-bit add, so that the loads, the LDS traffic and the MFMAs of
// one k step are ONE basic block.  Output tiles on the matrix edge run the same loop (workgroups that share a k slice
// through the L2 then keep the same pace; with the edge tiles on the tested loads the dW GEMM of cfg 4 lost 40 %):
// the rows of a k-contiguous operand beyond R are clamped to row R - 1, the columns of the other layout beyond R read on
// into the next row (at most 127 floats; the loop stops two k tiles = 32 rows before kend, so that is allocated memory
// whenever ld >= 8).  What those lanes fetch only reaches C rows / columns that are never stored.
template <bool KCONTIG>
__device__ __forceinline__ void tile_offsets(long long ld, int r0, int k0, int R, long long (&off)[NP]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    if constexpr (KCONTIG) {
      int r = r0 + t / KT + (256 / KT) * p;
      r = r < R ? r : R - 1;
      off[p] = static_cast<long long>(r) * ld + k0 + (t % KT) * 4;
    } else {
      off[p] = static_cast<long long>(k0 + (t >> 5) + 8 * p) * ld + r0 + (t & 31) * 4;
    }
  }
}
// The loads are issued as inline assembly: written as C++ the compiler sinks them down to the LDS stores that consume
// them (one basic block, single use), which exposes the whole memory latency; a fence does not hold them.  tile_arrived()
// is the matching wait -- it names the registers as read-write so that no use can be scheduled above it.
__device__ __forceinline__ void tile_issue(const float* base, long long (&off)[NP], long long step, f32x4 (&v)[NP]) {
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    // four floats in one request whatever the row pitch: global memory takes dword-aligned dwordx4 loads (K = 1677)
    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(v[p]) : "v"(base + off[p]));
    off[p] += step;
  }
}
__device__ __forceinline__ void tile_arrived(f32x4 (&a)[NP], f32x4 (&b)[NP]) {
  static_assert(NP == 2, "the operand list below is written for two float4 per thread and operand");
  asm volatile("s_waitcnt vmcnt(0)" : "+v"(a[0]), "+v"(a[1]), "+v"(b[0]), "+v"(b[1]) : : "memory");
}
template <bool KCONTIG>
__device__ __forceinline__ void store_tile_v(float* __restrict__ tile, const f32x4 (&v)[NP]) {
  float reg[4 * NP];
#pragma unroll
  for (int p = 0; p < NP; ++p)
#pragma unroll
    for (int j = 0; j < 4; ++j) reg[p * 4 + j] = v[p][j];
  store_tile<KCONTIG>(tile, reg);
}

// MFMA steps kk in [KLO, KHI) of one staged k tile for a wavefront's 2 x 2 tiles of 32 x 32: only the tiles named in
// LIVE (bit 2 i + j) -- a wavefront whose 32-row / 32-column blocks lie beyond M / N skips
// their products (N = 400 is 12.5 blocks: the weight-gradient GEMM [400, 65536] x [65536, 400] would otherwise run
// 512 x 512 outputs' worth of MFMAs for 400 x 400).
template <int KLO, int KHI, int LIVE>
__device__ __forceinline__ void mfma_steps(const float* __restrict__ as, const float* __restrict__ bs, int wm, int wn, int li,
                                           int lk, f32x16 (&acc)[2][2], int wm1, int wn1) {
#pragma unroll
  for (int kk = KLO; kk < KHI; kk += 2) {
    float a0 = 0.f, a1 = 0.f, b0 = 0.f, b1 = 0.f;
    if constexpr ((LIVE & 3) != 0) a0 = as[(kk + lk) * LDT + wm + li];
    if constexpr ((LIVE & 12) != 0) a1 = as[(kk + lk) * LDT + wm1 + li];
    if constexpr ((LIVE & 5) != 0) b0 = bs[(kk + lk) * LDT + wn + li];
    if constexpr ((LIVE & 10) != 0) b1 = bs[(kk + lk) * LDT + wn1 + li];
    if constexpr ((LIVE & 1) != 0) acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
    if constexpr ((LIVE & 2) != 0) acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
    if constexpr ((LIVE & 4) != 0) acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
    if constexpr ((LIVE & 8) != 0) acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
  }
}

// All k tiles but the last two: the tile after the current one is loaded without tests and parked in LDS[cur ^ 1] HALFWAY
// through the current tile's MFMAs (its stores issue in their shadow instead of after them), one barrier per tile.
// Leaves k0 / cur at the first tile the tested loop below has to finish (its operands are staged).
template <bool AK, bool BK_, int LIVE>
__device__ __forceinline__ void gemm_steady(const float* __restrict__ A, long long lda, const float* __restrict__ B,
                                            long long ldb, int m0, int n0, int M, int N, int kend, int& k0, int& cur,
                                            float (&As)[2][BK * LDT], float (&Bs)[2][BK * LDT], int wm, int wn, int li, int lk,
                                            f32x16 (&acc)[2][2]) {
  f32x4 va[NP], vb[NP];
  long long pa[NP], pb[NP];
  tile_offsets<AK>(lda, m0, k0 + BK, M, pa);
  tile_offsets<BK_>(ldb, n0, k0 + BK, N, pb);
  const long long step_a = AK ? BK : BK * lda, step_b = BK_ ? BK : BK * ldb;
  for (; k0 + 3 * BK <= kend; k0 += BK) {
    tile_issue(A, pa, step_a, va);
    tile_issue(B, pb, step_b, vb);
    mfma_steps<0, BK / 2, LIVE>(As[cur], Bs[cur], wm, wn, li, lk, acc, wm + 32, wn + 32);
    __builtin_amdgcn_sched_barrier(0);
    tile_arrived(va, vb);
    store_tile_v<AK>(As[cur ^ 1], va);
    store_tile_v<BK_>(Bs[cur ^ 1], vb);
    mfma_steps<BK / 2, BK, LIVE>(As[cur], Bs[cur], wm, wn, li, lk, acc, wm + 32, wn + 32);
    __syncthreads();
    cur ^= 1;
  }
}

// Narrow companion of gemm_f32_kernel for the last 32 * NT (<= 64) output columns: N = 400 is 3 full 128-column
// tiles plus 16 columns, and a fourth full tile would spend 22% of the MFMA time on padding.  The four wavefronts
// stack along M (32 rows each) and every wavefront computes NT 32x32 MFMA tiles; same operand staging.
template <bool A_KCONTIG, bool B_KCONTIG, int NT>
__device__ __forceinline__ void narrow_tile(const float* __restrict__ A, const long long lda, const float* __restrict__ B,
                                            const long long ldb, float* __restrict__ C, const long long ldc, const int M,
                                            const int N, const int K, const int n0, const float* __restrict__ bias,
                                            const int act, const bool vec_a, const bool vec_b, const Epi& epi, const int m0,
                                            float (&As)[2][BK * LDT], float (&Bs)[2][BK * LDT]) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int wm = wid * 32;
  const int li = lane & 31, lk = lane >> 5;
  const int nlim = (n0 + 32 * NT < N) ? n0 + 32 * NT : N;      // B rows beyond the narrow tile are not fetched
  f32x16 acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
  // The epilogue's extra operands are fetched NOW: this kernel runs a handful of k tiles (K = 64 for the SASRec
  // projections), so a load issued after the last MFMA is a full memory round trip that nothing hides (measured: the
  // fused launches took 270 us instead of 126).  They arrive while the operand tiles do.
  f32x16 eres[NT], emask[NT];
  float erow[16];
  const bool has_res = epi.res != nullptr, has_mask = epi.mask != nullptr, has_rs = epi.rowscale != nullptr;
  if (has_res || has_mask) {
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int col = n0 + j * 32 + li;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = m0 + wm + (r & 3) + 8 * (r >> 2) + 4 * lk;
        const bool ok = row < M && col < N;
        eres[j][r] = (has_res && ok) ? epi.res[static_cast<long long>(row) * epi.ldres + col] : 0.f;
        emask[j][r] = (has_mask && ok) ? epi.mask[static_cast<long long>(row) * epi.ldmask + col] : 1.f;
      }
    }
  }
  if (has_rs) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = m0 + wm + (r & 3) + 8 * (r >> 2) + 4 * lk;
      erow[r] = row < M ? epi.rowscale[row] : 0.f;
    }
  }
  float ra[4 * NP], rb[4 * NP];
  load_tile<A_KCONTIG>(A, lda, m0, 0, M, K, vec_a, ra);
  load_tile<B_KCONTIG>(B, ldb, n0, 0, nlim, K, vec_b, rb);
  store_tile<A_KCONTIG>(As[0], ra);
  store_tile<B_KCONTIG>(Bs[0], rb);
  __syncthreads();
  int cur = 0;
  for (int k0 = 0; k0 < K; k0 += BK) {
    const bool more = k0 + BK < K;
    if (more) {
      load_tile<A_KCONTIG>(A, lda, m0, k0 + BK, M, K, vec_a, ra);
      load_tile<B_KCONTIG>(B, ldb, n0, k0 + BK, nlim, K, vec_b, rb);
    }
    const float* as = As[cur];
    const float* bs = Bs[cur];
#pragma unroll
    for (int kk = 0; kk < BK; kk += 2) {
      const float a0 = as[(kk + lk) * LDT + wm + li];
#pragma unroll
      for (int j = 0; j < NT; ++j)
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, bs[(kk + lk) * LDT + j * 32 + li], acc[j], 0, 0, 0);
    }
    if (more) {
      store_tile<A_KCONTIG>(As[cur ^ 1], ra);
      store_tile<B_KCONTIG>(Bs[cur ^ 1], rb);
    }
    __syncthreads();
    cur ^= 1;
  }
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int col = n0 + j * 32 + li;
    if (col >= N) continue;
    const float bv = bias != nullptr ? bias[col] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = m0 + wm + (r & 3) + 8 * (r >> 2) + 4 * lk;
      if (row < M) {
        float v = acc[j][r] + bv;
        if (act == 1) v = v > 0.f ? v : 0.f;
        if (has_mask) v = emask[j][r] > 0.f ? v : 0.f;
        if (has_res) v += eres[j][r];
        v += epi_fm_term(epi, row, col);
        if (has_rs) v *= erow[r];
        C[static_cast<long long>(row) * ldc + col] = v;
      }
    }
  }
}

template <bool A_KCONTIG, bool B_KCONTIG, int NT>
__global__ __launch_bounds__(256) void gemm_f32_narrow_kernel(const float* __restrict__ A, const long long lda,
                                                              const float* __restrict__ B, const long long ldb,
                                                              float* __restrict__ C, const long long ldc, const int M,
                                                              const int N, const int K, const int n0,
                                                              const float* __restrict__ bias, const int act,
                                                              const bool vec_a, const bool vec_b, const Epi epi) {
  __shared__ float As[2][BK * LDT];
  __shared__ float Bs[2][BK * LDT];
  narrow_tile<A_KCONTIG, B_KCONTIG, NT>(A, lda, B, ldb, C, ldc, M, N, K, n0, bias, act, vec_a, vec_b, epi,
                                        static_cast<int>(blockIdx.x) * BM, As, Bs);
}

// C[M,N] (+bias, act) = A(M,K) * B(K,N); with splits > 1 a workgroup computes one K slice of its tile
// (then C points at the slice's private [M,N] buffer: C + z * M * N, no epilogue math).
template <bool A_KCONTIG, bool B_KCONTIG>
__global__ __launch_bounds__(256, 4) void gemm_f32_kernel(const float* __restrict__ A, const long long lda,
                                                       const float* __restrict__ B, const long long ldb,
                                                       float* __restrict__ C, const long long ldc, const int M,
                                                       const int N, const int K, const int k_per_split,
                                                       const float* __restrict__ bias, const int act,
                                                       const bool vec_a, const bool vec_b, const int tiles_m,
                                                       const int tiles_n, const int splits, const int narrow_from,
                                                       const int narrow_nt, const Epi epi) {
  __shared__ float As[2][BK * LDT];
  __shared__ float Bs[2][BK * LDT];
  // The first `narrow_from` workgroups compute the narrow tail (the last <= 64 columns behind tiles_n full column tiles) of
  // row block blockIdx.x with the narrow kernel's body instead of a launch of their own: their k loop is bound by memory
  // latency (one 32 x 32 tile per wavefront), so they start first and run BESIDE the full tiles, which keep the MFMA pipes
  // busy meanwhile.  (Launched last they began in the final, half-empty round and outlived it: 766 vs 786 us only.)
  if (static_cast<int>(blockIdx.x) < narrow_from) {
    const int m0n = static_cast<int>(blockIdx.x) * BM;
    if (narrow_nt == 1) narrow_tile<A_KCONTIG, B_KCONTIG, 1>(A, lda, B, ldb, C, ldc, M, N, K, tiles_n * BN, bias, act, vec_a, vec_b, epi, m0n, As, Bs);
    else narrow_tile<A_KCONTIG, B_KCONTIG, 2>(A, lda, B, ldb, C, ldc, M, N, K, tiles_n * BN, bias, act, vec_a, vec_b, epi, m0n, As, Bs);
    return;
  }
  int tm_i, tn_j, z = 0;
  if (splits == 1) {
    xcd_tile(static_cast<int>(blockIdx.x) - narrow_from, tiles_m, tiles_n, &tm_i, &tn_j);
  } else {
    // K split over `splits` workgroups per tile, one flat launch: the tiles with 128 x 128 real outputs first (every K slice
    // of them), the tiles on the matrix edge after them.  All workgroups are resident at once and the dispatcher deals
    // them out in launch order, so the full tiles spread evenly (the host sizes `splits` for two of them per CU) and the
    // edge tiles -- a fraction of the MFMA work -- land on top as third workgroups instead of displacing full ones.
    const int tm_f = M / BM, tn_f = N / BN, n_full = tm_f * tn_f, n_edge = tiles_m * tiles_n - n_full;
    const int L = static_cast<int>(blockIdx.x) - narrow_from;
    if (L < n_full * splits) {
      z = L / n_full;
      const int f = L % n_full;
      tm_i = f / tn_f;
      tn_j = f % tn_f;
    } else {
      const int e = L - n_full * splits;
      z = e / n_edge;
      const int q = e % n_edge, right = (tiles_n > tn_f) ? tm_f : 0;     // the right-hand column strip, then the bottom row
      if (q < right) { tm_i = q; tn_j = tn_f; }
      else { tm_i = tm_f; tn_j = q - right; }
    }
  }
  const int m0 = tm_i * BM, n0 = tn_j * BN;
  const int kbeg = z * k_per_split;
  const int kend = (kbeg + k_per_split < K) ? kbeg + k_per_split : K;
  if (splits > 1) C += static_cast<long long>(z) * M * ldc;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int li = lane & 31, lk = lane >> 5;
  const WavePlace wp = place_dealt(wid, M - m0, N - n0);
  const int wm = wp.wm, wn = wp.wn, live = wp.live;
  f32x16 acc[2][2];
  zero_acc(acc);

  float ra[4 * NP], rb[4 * NP];
  load_tile<A_KCONTIG>(A, lda, m0, kbeg, M, kend, vec_a, ra);
  load_tile<B_KCONTIG>(B, ldb, n0, kbeg, N, kend, vec_b, rb);
  store_tile<A_KCONTIG>(As[0], ra);
  store_tile<B_KCONTIG>(Bs[0], rb);
  __syncthreads();
  int cur = 0;
  int k0 = kbeg;
  if ((A_KCONTIG || lda >= 8) && (B_KCONTIG || ldb >= 8)) {     // (see tile_offsets: how far an edge tile reads on)
    with_live(live, [&](auto live_c) {
      gemm_steady<A_KCONTIG, B_KCONTIG, decltype(live_c)::value>(A, lda, B, ldb, m0, n0, M, N, kend, k0, cur, As, Bs, wm, wn, li,
                                                                 lk, acc);
    });
  }
  for (; k0 < kend; k0 += BK) {
    const bool more = k0 + BK < kend;
    if (more) {                                    // next tile's HBM reads fly under this tile's MFMAs
      load_tile<A_KCONTIG>(A, lda, m0, k0 + BK, M, kend, vec_a, ra);
      load_tile<B_KCONTIG>(B, ldb, n0, k0 + BK, N, kend, vec_b, rb);
    }
    // (the last two k tiles run all four products: tiles that are not live read a clamped block and are never stored)
    mfma_steps<0, BK, 15>(As[cur], Bs[cur], wm, wn, li, lk, acc, wm < 96 ? wm + 32 : 96, wn < 96 ? wn + 32 : 96);
    if (more) {
      store_tile<A_KCONTIG>(As[cur ^ 1], ra);
      store_tile<B_KCONTIG>(Bs[cur ^ 1], rb);
    }
    __syncthreads();
    cur ^= 1;
  }
  gemm_epilogue(acc, m0, n0, wm, wn, li, lk, live, M, N, C, ldc, bias, act, splits, epi);
}

}  // namespace rbx
