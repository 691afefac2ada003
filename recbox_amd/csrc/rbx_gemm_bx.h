// rbx_gemm_bx.h -- f32 GEMM on the bf16 matrix cores: operands split three ways, six products.  Included by rbx_dense.hip
// behind rbx_gemm_tile.h.
//
// CDNA4 runs v_mfma_f32_32x32x2_f32 at the f32 VECTOR rate (157 TF); its bf16 MFMAs are 16x that (2.5 PF) and accumulate
// in f32.  Every f32 x = h + m + l with bf16 h = rn(x), m = rn(x - h), l = rn(x - h - m) (3 x 8 significant bits:
// |x - h - m - l| <= 2^-24 |x|), so
//     a b = ah bh + (ah bm + am bh) + (ah bl + al bh + am bm) + O(2^-24 |a b|):
// six v_mfma_f32_32x32x16_bf16 per 16 k (192 cycles) instead of eight f32 MFMAs (512 cycles), with an error per product of
// the size of ONE f32 rounding -- the sums carry the same ~sqrt(K) 2^-24 as the f32 kernel's (tests: the same tolerances
// against float64).  bf16 has f32's exponent range: nothing overflows that f32 would not; non-finite inputs come out as
// NaN (inf - inf in the split), f32 denormals lose their low parts.
// Form: y = x W^T and dx = dy W, i.e. A [M, K] row-major activations against weights.  The WEIGHTS are split once per call
// by rbx_split_bf16 into three k-major bf16 planes (transposed for dx), which the caller registers for the duration of the
// GEMM call (rbx_split_register); the activations are split on their way from registers to LDS (v_cvt_pk_bf16_f32, 4.5 VALU
// ops per element beside the MFMAs).  LDS: three bf16 planes per operand, rows k-major in 80-byte pitch (conflict-free
// b128 reads).  The weight-gradient GEMM (both operands batch-major activations): gemm_bxt_kernel further down.
// Three kernels: gemm_bx6_kernel (128 x 128 tile, two barriers per k tile), and gemm_bxp_kernel / gemm_bxt_kernel
// (256 x 128 tile, one barrier per k tile, two tiles prefetched).  The fragment reads and the six products are shared.
#pragma once
#include <type_traits>
#include "rbx_gemm_tile.h"

namespace rbx {

typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef float f32x4u_t __attribute__((ext_vector_type(4), aligned(4)));      // a dwordx4 load needs dword alignment only
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
constexpr int SBK = 32;                 // k per staged tile: two MFMA steps of 16
constexpr int SLD = SBK + 8;            // LDS row pitch, bf16 elements
constexpr int SPLANE = BM * SLD;        // one plane of one operand

__device__ __forceinline__ void split2(f32x2_t x, unsigned& h, unsigned& m, unsigned& l) {
  const bf16x2_t hb = __builtin_convertvector(x, bf16x2_t);
  x -= __builtin_convertvector(hb, f32x2_t);
  const bf16x2_t mb = __builtin_convertvector(x, bf16x2_t);
  x -= __builtin_convertvector(mb, f32x2_t);
  const bf16x2_t lb = __builtin_convertvector(x, bf16x2_t);
  h = __builtin_bit_cast(unsigned, hb);
  m = __builtin_bit_cast(unsigned, mb);
  l = __builtin_bit_cast(unsigned, lb);
}

// ---- what the three k loops share: the fragments of one MFMA step and its six products --------------------------------------
// The wavefront's 2 x 3 A and 2 x 3 B fragments (32-row block i, plane q) of one k step of 16 out of LDS planes of
// PLANE_A / PLANE_B elements with row pitch LD; ap / bp point at the lane's row and k group of plane 0, block 0.  Only the
// fragments some live tile needs: the others lie outside the tile.
template <int LIVE, int PLANE_A, int PLANE_B, int LD>
__device__ __forceinline__ void bx_frags(const unsigned short* __restrict__ ap, const unsigned short* __restrict__ bp,
                                         const int ks_off, bf16x8_t (&a)[2][3], bf16x8_t (&b)[2][3]) {
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      if ((LIVE >> (2 * i)) & 3) a[i][q] = *reinterpret_cast<const bf16x8_t*>(ap + q * PLANE_A + i * 32 * LD + ks_off);
      if ((LIVE >> i) & 5) b[i][q] = *reinterpret_cast<const bf16x8_t*>(bp + q * PLANE_B + i * 32 * LD + ks_off);
    }
}
// one of the six products, plane QA of A against plane QB of B, for every live output tile: the four tiles' chains
// interleaved (a dependent MFMA waits for its predecessor)
template <int LIVE, int QA, int QB>
__device__ __forceinline__ void bx_term(const bf16x8_t (&a)[2][3], const bf16x8_t (&b)[2][3], f32x16 (&acc)[2][2]) {
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
      if ((LIVE >> (2 * i + j)) & 1) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i][QA], b[j][QB], acc[i][j], 0, 0, 0);
}
// the six products in ascending size, in two halves (the pipelined loop parks the next tile between them)
template <int LIVE>
__device__ __forceinline__ void bx_terms_low(const bf16x8_t (&a)[2][3], const bf16x8_t (&b)[2][3], f32x16 (&acc)[2][2]) {
  bx_term<LIVE, 2, 0>(a, b, acc);
  bx_term<LIVE, 0, 2>(a, b, acc);
  bx_term<LIVE, 1, 1>(a, b, acc);
}
template <int LIVE>
__device__ __forceinline__ void bx_terms_high(const bf16x8_t (&a)[2][3], const bf16x8_t (&b)[2][3], f32x16 (&acc)[2][2]) {
  bx_term<LIVE, 1, 0>(a, b, acc);
  bx_term<LIVE, 0, 1>(a, b, acc);
  bx_term<LIVE, 0, 0>(a, b, acc);
}

// ---- 128 x 128 tile, two barriers per k tile of 32 -----------------------------------------------------------------------------
// A tile [128, SBK] of f32 activations, global -> registers: thread t takes k = 4 (t % 8) .. + 3 of rows t / 8 + 32 p.
// k beyond K reads as zero, rows beyond M are clamped (their products only reach outputs that are never stored).
__device__ __forceinline__ void bx6_load_a(const float* __restrict__ A, long long lda, int m0, int k0, int M, int K,
                                           f32x4u_t (&v)[4]) {
  const int t = threadIdx.x;
  const int k = k0 + (t & 7) * 4;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    int r = m0 + (t >> 3) + 32 * p;
    r = r < M ? r : M - 1;
    const float* src = A + static_cast<long long>(r) * lda + k;
    if (k + 3 < K) {
      v[p] = *reinterpret_cast<const f32x4u_t*>(src);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[p][j] = (k + j < K) ? src[j] : 0.f;
    }
  }
}
__device__ __forceinline__ void bx6_store_a(unsigned short* __restrict__ tile, const f32x4u_t (&v)[4]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    unsigned h0, m0, l0, h1, m1, l1;
    split2(f32x2_t{v[p][0], v[p][1]}, h0, m0, l0);
    split2(f32x2_t{v[p][2], v[p][3]}, h1, m1, l1);
    unsigned short* dst = tile + ((t >> 3) + 32 * p) * SLD + (t & 7) * 4;
    *reinterpret_cast<uint2*>(dst) = make_uint2(h0, h1);
    *reinterpret_cast<uint2*>(dst + SPLANE) = make_uint2(m0, m1);
    *reinterpret_cast<uint2*>(dst + 2 * SPLANE) = make_uint2(l0, l1);
  }
}
// B tile [128 rows (output columns), SBK] of the pre-split weights.  Layout of the planes (rbx_split_bf16): per row, per group
// of 8 k, the three planes' 16 bytes side by side -- [row][kp / 8][3][8] bf16, kp a multiple of SBK (zero-filled) -- so that a
// row's share of a k tile is 192 contiguous bytes (with one [rows][kp] array per plane it was three 64-byte pieces: three
// times the requests of the f32 original, and the kernel ran at 100 TF instead of 167).  Thread t takes the 16-byte chunks
// t + 256 i, i < 6: chunk j = row j / 12, piece j % 12 = 3 (k group) + plane.
__device__ __forceinline__ void bx6_load_b(const unsigned short* __restrict__ Bp, int kp, int n0, int k0, int N, u32x4_t (&v)[6]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const int j = t + 256 * i;
    int r = n0 + j / 12;
    r = r < N ? r : N - 1;
    v[i] = *reinterpret_cast<const u32x4_t*>(Bp + static_cast<long long>(r) * 3 * kp + (k0 >> 3) * 24 + (j % 12) * 8);
  }
}
__device__ __forceinline__ void bx6_store_b(unsigned short* __restrict__ tile, const u32x4_t (&v)[6]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const int j = t + 256 * i;
    const int c = j % 12;
    *reinterpret_cast<u32x4_t*>(tile + (c % 3) * SPLANE + (j / 12) * SLD + (c / 3) * 8) = v[i];
  }
}

template <int LIVE>
__device__ __forceinline__ void bx6_loop(const float* __restrict__ A, const long long lda, const unsigned short* __restrict__ Bp,
                                         const int kp, const int m0, const int n0, const int M, const int N, const int K,
                                         unsigned short* __restrict__ As, unsigned short* __restrict__ Bs, const int wm,
                                         const int wn, const int li, const int lk, f32x16 (&acc)[2][2]) {
  f32x4u_t ra[4];
  u32x4_t rb[6];
  bx6_load_a(A, lda, m0, 0, M, K, ra);
  bx6_load_b(Bp, kp, n0, 0, N, rb);
  const unsigned short* ap = As + (wm + li) * SLD + 8 * lk;
  const unsigned short* bp = Bs + (wn + li) * SLD + 8 * lk;
  for (int k0 = 0; k0 < K; k0 += SBK) {
    bx6_store_a(As, ra);
    bx6_store_b(Bs, rb);
    if (k0 + SBK < K) {                           // the next tile's reads fly under the barrier and this tile's MFMAs
      bx6_load_a(A, lda, m0, k0 + SBK, M, K, ra);
      bx6_load_b(Bp, kp, n0, k0 + SBK, N, rb);
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < SBK / 16; ++ks) {
      bf16x8_t a[2][3], b[2][3];
      bx_frags<LIVE, SPLANE, SPLANE, SLD>(ap, bp, ks * 16, a, b);
      bx_terms_low<LIVE>(a, b, acc);
      bx_terms_high<LIVE>(a, b, acc);
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256, 2) void gemm_bx6_kernel(const float* __restrict__ A, const long long lda,
                                                          const unsigned short* __restrict__ Bp, const int kp,
                                                          float* __restrict__ C, const long long ldc, const int M, const int N,
                                                          const int K, const float* __restrict__ bias, const int act,
                                                          const int tiles_m, const int tiles_n, const Epi epi) {
  __shared__ __attribute__((aligned(16))) unsigned short As[3 * SPLANE];
  __shared__ __attribute__((aligned(16))) unsigned short Bs[3 * SPLANE];
  int tm_i, tn_j;
  xcd_tile(static_cast<int>(blockIdx.x), tiles_m, tiles_n, &tm_i, &tn_j);
  const int m0 = tm_i * BM, n0 = tn_j * BN;
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  const int li = lane & 31, lk = lane >> 5;
  const WavePlace wp = place_dealt(wid, M - m0, N - n0);
  const int wm = wp.wm, wn = wp.wn, live = wp.live;
  f32x16 acc[2][2];
  zero_acc(acc);
  with_live(live, [&](auto live_c) {
    bx6_loop<decltype(live_c)::value>(A, lda, Bp, kp, m0, n0, M, N, K, As, Bs, wm, wn, li, lk, acc);
  });
  gemm_epilogue(acc, m0, n0, wm, wn, li, lk, live, M, N, C, ldc, bias, act, 1, epi);
}

// ---- the same GEMM with a 256 x 128 tile, pipelined ----------------------------------------------------------------------------
// gemm_bx6_kernel above runs at 0.34-0.38 of the bf16 pipes whatever its loop looks like (a one-barrier, double-buffered
// form of the same 128 x 128 tile measured 157 vs 160 TF): at six MFMAs per 16 k a 128 x 128 tile asks the L2 for 20 KB
// (8 KB of f32 activations + 12 KB of weight planes) per 768 MFMA cycles -- 16 TB/s over the chip at full rate, more than
// the L2s deliver; it is the plain-bf16 ladder of the guide again (128^2 tiles: 0.36 of peak).  Here a workgroup of EIGHT
// wavefronts owns 256 rows x 128 columns (the weight tile amortised over twice the rows: 28 KB per 2 x the products), k tiles
// of 16 in two LDS buffers, ONE barrier per tile: the tile after the current one is split and parked in the other buffer
// between the two halves of the current tile's MFMAs, the loads of the tile after that issued right behind.
constexpr int PBK = 16;                 // k per tile: one MFMA step
constexpr int PLD = PBK + 8;            // LDS row pitch, bf16 elements (48 bytes: conflict-free b128 reads of 16 rows)
constexpr int PBM = 256;                // rows of the workgroup's tile
constexpr int PTHREADS = 512;
constexpr int PPLANE_A = PBM * PLD, PPLANE_B = BN * PLD;
constexpr int PBUF_A = 3 * PPLANE_A, PBUF_B = 3 * PPLANE_B;
constexpr int kBxPipeLds = 2 * (PBUF_A + PBUF_B) * 2;       // bytes: 2 x (A 36 KB + B 18 KB) = 108 KB

// A tile [256, 16]: thread t takes k = 4 (t % 4) .. + 3 of rows t / 4 and 128 + t / 4
template <bool GUARD>
__device__ __forceinline__ void bxp_load_a(const float* __restrict__ A, long long lda, int m0, int k0, int M, int K,
                                           f32x4u_t (&v)[2]) {
  const int t = threadIdx.x;
  const int k = k0 + (t & 3) * 4;
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    int r = m0 + (t >> 2) + 128 * p;
    r = r < M ? r : M - 1;
    const float* src = A + static_cast<long long>(r) * lda + k;
    if (!GUARD || k + 3 < K) {
      v[p] = *reinterpret_cast<const f32x4u_t*>(src);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[p][j] = (k + j < K) ? src[j] : 0.f;
    }
  }
}
__device__ __forceinline__ void bxp_store_a(unsigned short* __restrict__ buf, const f32x4u_t (&v)[2]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    unsigned h0, m0, l0, h1, m1, l1;
    split2(f32x2_t{v[p][0], v[p][1]}, h0, m0, l0);
    split2(f32x2_t{v[p][2], v[p][3]}, h1, m1, l1);
    unsigned short* dst = buf + ((t >> 2) + 128 * p) * PLD + (t & 3) * 4;
    *reinterpret_cast<uint2*>(dst) = make_uint2(h0, h1);
    *reinterpret_cast<uint2*>(dst + PPLANE_A) = make_uint2(m0, m1);
    *reinterpret_cast<uint2*>(dst + 2 * PPLANE_A) = make_uint2(l0, l1);
  }
}
// B tile [128 rows, 16 k] of the interleaved planes: 96 contiguous bytes per row = 768 chunks of 16 bytes; thread t takes
// chunk t and, the first 256 threads, chunk 512 + t
__device__ __forceinline__ void bxp_load_b(const unsigned short* __restrict__ Bp, int kp, int n0, int k0, int N, u32x4_t (&v)[2]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    int j = t + PTHREADS * i;
    j = j < 768 ? j : t;                   // (the upper half of the second round repeats its first chunk: no branch)
    int r = n0 + j / 6;
    r = r < N ? r : N - 1;
    v[i] = *reinterpret_cast<const u32x4_t*>(Bp + static_cast<long long>(r) * 3 * kp + (k0 >> 3) * 24 + (j % 6) * 8);
  }
}
__device__ __forceinline__ void bxp_store_b(unsigned short* __restrict__ buf, const u32x4_t (&v)[2]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    int j = t + PTHREADS * i;
    j = j < 768 ? j : t;
    const int c = j % 6;
    *reinterpret_cast<u32x4_t*>(buf + (c % 3) * PPLANE_B + (j / 6) * PLD + (c / 3) * 8) = v[i];
  }
}


template <int LIVE>
__device__ __forceinline__ void bxp_loop(const float* __restrict__ A, const long long lda, const unsigned short* __restrict__ Bp,
                                         const int kp, const int m0, const int n0, const int M, const int N, const int K,
                                         unsigned short* __restrict__ As, unsigned short* __restrict__ Bs, const int wm,
                                         const int wn, const int li, const int lk, f32x16 (&acc)[2][2]) {
  // Two register sets: the loads of a tile are issued two iterations ahead of its split (one ahead: 46 % of the wavefront
  // cycles parked (PMC), 158 TF at 8192^3; two: 184) -- set (t + 1) % 2 holds tile t + 1 when iteration t starts
  f32x4u_t ra[2][2];
  u32x4_t rb[2][2];
  const int kt = (K + PBK - 1) / PBK;              // tiles; the weight planes are zero-filled up to a multiple of 32;
  auto fetch = [&](int tile, auto set_c) {
    constexpr int set = decltype(set_c)::value;
    if ((tile + 1) * PBK <= K) bxp_load_a<false>(A, lda, m0, tile * PBK, M, K, ra[set]);
    else bxp_load_a<true>(A, lda, m0, tile * PBK, M, K, ra[set]);
    bxp_load_b(Bp, kp, n0, tile * PBK, N, rb[set]);
  };
  fetch(0, std::integral_constant<int, 0>{});
  bxp_store_a(As, ra[0]);
  bxp_store_b(Bs, rb[0]);
  if (kt > 1) fetch(1, std::integral_constant<int, 1>{});
  if (kt > 2) fetch(2, std::integral_constant<int, 0>{});
  __syncthreads();
  const int aoff = (wm + li) * PLD + 8 * lk, boff = (wn + li) * PLD + 8 * lk;
  auto step = [&](int t, int cur, auto set_c) {
    constexpr int set = decltype(set_c)::value;    // the set that holds tile t + 1
    bf16x8_t a[2][3], b[2][3];
    bx_frags<LIVE, PPLANE_A, PPLANE_B, PLD>(As + cur * PBUF_A + aoff, Bs + cur * PBUF_B + boff, 0, a, b);
    bx_terms_low<LIVE>(a, b, acc);
    if (t + 1 < kt) {                              // tile t + 1 -> the other buffer, in the shadow of this tile's MFMAs
      bxp_store_a(As + (cur ^ 1) * PBUF_A, ra[set]);
      bxp_store_b(Bs + (cur ^ 1) * PBUF_B, rb[set]);
    }
    if (t + 3 < kt) fetch(t + 3, set_c);           // the tile two iterations ahead into the set just emptied
    bx_terms_high<LIVE>(a, b, acc);
    __syncthreads();
  };
  // Steady state (every tile up to t + 3 lies inside K: no tests): the same step as ONE basic block, with the order the
  // instructions should issue in spelled out -- the twelve LDS reads first, then an MFMA with four of the split's VALU
  // ops / one LDS store / one global load in each of its shadows.  Left to the compiler the whole split lands behind the
  // MFMAs: 184 TF at 8192^3 and 585 us for the layer-1 forward, against 196-198 TF and 530 us (profiles/r03/INDEX.md).
  auto steady = [&](int t, int cur, auto set_c) {
    constexpr int set = decltype(set_c)::value;
    bf16x8_t a[2][3], b[2][3];
    bx_frags<LIVE, PPLANE_A, PPLANE_B, PLD>(As + cur * PBUF_A + aoff, Bs + cur * PBUF_B + boff, 0, a, b);
    bx_terms_low<LIVE>(a, b, acc);
    bxp_store_a(As + (cur ^ 1) * PBUF_A, ra[set]);
    bxp_store_b(Bs + (cur ^ 1) * PBUF_B, rb[set]);
    bxp_load_a<false>(A, lda, m0, (t + 3) * PBK, M, K, ra[set]);
    bxp_load_b(Bp, kp, n0, (t + 3) * PBK, N, rb[set]);
    bx_terms_high<LIVE>(a, b, acc);
    __builtin_amdgcn_sched_group_barrier(0x100, 12, 0);                    // DS reads
#pragma unroll
    for (int g = 0; g < 12; ++g) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                   // MFMA
      __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);                   // VALU
    }
#pragma unroll
    for (int g = 0; g < 8; ++g) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);                   // DS write
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);                   // VMEM read
    }
    __syncthreads();
  };
  int t = 0;
  if constexpr (LIVE == 15) {
    while ((t + 5) * PBK <= K) {      // two steps per round: tiles t + 3 and t + 4 are read without tests
      steady(t, 0, std::integral_constant<int, 1>{});
      steady(t + 1, 1, std::integral_constant<int, 0>{});
      t += 2;
    }
  }
  // the rest (and edge tiles): the tested step; t is even here, so LDS buffer and register set line up
  for (; t < kt; t += 2) {
    step(t, 0, std::integral_constant<int, 1>{});
    if (t + 1 < kt) step(t + 1, 1, std::integral_constant<int, 0>{});
  }
}

__global__ __launch_bounds__(PTHREADS, 1) void gemm_bxp_kernel(const float* __restrict__ A, const long long lda,
                                                               const unsigned short* __restrict__ Bp, const int kp,
                                                               float* __restrict__ C, const long long ldc, const int M,
                                                               const int N, const int K, const float* __restrict__ bias,
                                                               const int act, const int tiles_m, const int tiles_n,
                                                               const Epi epi) {
  extern __shared__ __attribute__((aligned(16))) unsigned short bxp_lds[];          // kBxPipeLds
  unsigned short* As = bxp_lds;
  unsigned short* Bs = bxp_lds + 2 * PBUF_A;
  int tm_i, tn_j;
  xcd_tile(static_cast<int>(blockIdx.x), tiles_m, tiles_n, &tm_i, &tn_j);
  const int m0 = tm_i * PBM, n0 = tn_j * BN;
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  const int li = lane & 31, lk = lane >> 5;
  const WavePlace wp = place_plain(wid, M - m0, N - n0);
  const int wm = wp.wm, wn = wp.wn, live = wp.live;
  f32x16 acc[2][2];
  zero_acc(acc);
  with_live(live, [&](auto live_c) {
    bxp_loop<decltype(live_c)::value>(A, lda, Bp, kp, m0, n0, M, N, K, As, Bs, wm, wn, li, lk, acc);
  });
  gemm_epilogue(acc, m0, n0, wm, wn, li, lk, live, M, N, C, ldc, bias, act, 1, epi, PBM);
}

// ---- the weight-gradient GEMM dW = dy^T x on the same pipes --------------------------------------------------------------------
// Both operands are batch-major activations: A(i, kk) = dy[kk, i], B(kk, col) = x[kk, col] with the reduction index kk = the
// sample.  Same 256 x 128 x 16 tiles, LDS layout, MFMA phase and prefetch depth as gemm_bxp_kernel; what differs is the
// staging -- a lane reads ONE output row / column (dword loads: 64 consecutive floats of a sample's row per wavefront) for
// pairs of consecutive samples, so that a pair is one packed bf16x2 word of a k-major LDS row (b32 stores) -- both operands
// split in the kernel, and the K (batch) range split over workgroups into a workspace (splitk_reduce_kernel: fixed order).
template <bool GUARD>
__device__ __forceinline__ void bxt_load_a(const float* __restrict__ A, long long lda, int m0, int k0, int M, int kend,
                                           float (&v)[8]) {
  const int t = threadIdx.x;
  int i = m0 + (t & 255);
  i = i < M ? i : M - 1;
  const int kk = k0 + 8 * (t >> 8);
  const float* src = A + static_cast<long long>(kk) * lda + i;
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = (!GUARD || kk + e < kend) ? src[static_cast<long long>(e) * lda] : 0.f;
}
__device__ __forceinline__ void bxt_store_a(unsigned short* __restrict__ buf, const float (&v)[8]) {
  const int t = threadIdx.x;
  unsigned* dst = reinterpret_cast<unsigned*>(buf + (t & 255) * PLD + 8 * (t >> 8));
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    unsigned h, m, l;
    split2(f32x2_t{v[2 * j], v[2 * j + 1]}, h, m, l);
    dst[j] = h;
    dst[j + PPLANE_A / 2] = m;
    dst[j + PPLANE_A] = l;
  }
}
// B tile [128 col, 16 kk]: thread t takes col = t % 128 and the two sample pairs of kk in [4 (t / 128), + 4)
template <bool GUARD>
__device__ __forceinline__ void bxt_load_b(const float* __restrict__ B, long long ldb, int n0, int k0, int N, int kend,
                                           float (&v)[4]) {
  const int t = threadIdx.x;
  int c = n0 + (t & 127);
  c = c < N ? c : N - 1;
  const int kk = k0 + 4 * (t >> 7);
  const float* src = B + static_cast<long long>(kk) * ldb + c;
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = (!GUARD || kk + e < kend) ? src[static_cast<long long>(e) * ldb] : 0.f;
}
__device__ __forceinline__ void bxt_store_b(unsigned short* __restrict__ buf, const float (&v)[4]) {
  const int t = threadIdx.x;
  unsigned* dst = reinterpret_cast<unsigned*>(buf + (t & 127) * PLD + 4 * (t >> 7));
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    unsigned h, m, l;
    split2(f32x2_t{v[2 * j], v[2 * j + 1]}, h, m, l);
    dst[j] = h;
    dst[j + PPLANE_B / 2] = m;
    dst[j + PPLANE_B] = l;
  }
}


template <int LIVE>
__device__ __forceinline__ void bxt_loop(const float* __restrict__ A, const long long lda, const float* __restrict__ B,
                                         const long long ldb, const int m0, const int n0, const int M, const int N,
                                         const int kbeg, const int kend, unsigned short* __restrict__ As,
                                         unsigned short* __restrict__ Bs, const int wm, const int wn, const int li, const int lk,
                                         f32x16 (&acc)[2][2]) {
  float ra[2][8], rb[2][4];
  const int kt = (kend - kbeg + PBK - 1) / PBK;;
  auto fetch = [&](int tile, auto set_c) {
    constexpr int set = decltype(set_c)::value;
    bxt_load_a<true>(A, lda, m0, kbeg + tile * PBK, M, kend, ra[set]);
    bxt_load_b<true>(B, ldb, n0, kbeg + tile * PBK, N, kend, rb[set]);
  };
  fetch(0, std::integral_constant<int, 0>{});
  bxt_store_a(As, ra[0]);
  bxt_store_b(Bs, rb[0]);
  if (kt > 1) fetch(1, std::integral_constant<int, 1>{});
  if (kt > 2) fetch(2, std::integral_constant<int, 0>{});
  __syncthreads();
  const int aoff = (wm + li) * PLD + 8 * lk, boff = (wn + li) * PLD + 8 * lk;
  auto step = [&](int t, int cur, auto set_c) {
    constexpr int set = decltype(set_c)::value;    // the set that holds tile t + 1
    bf16x8_t a[2][3], b[2][3];
    bx_frags<LIVE, PPLANE_A, PPLANE_B, PLD>(As + cur * PBUF_A + aoff, Bs + cur * PBUF_B + boff, 0, a, b);
    bx_terms_low<LIVE>(a, b, acc);
    if (t + 1 < kt) {                              // tile t + 1 -> the other buffer, in the shadow of this tile's MFMAs
      bxt_store_a(As + (cur ^ 1) * PBUF_A, ra[set]);
      bxt_store_b(Bs + (cur ^ 1) * PBUF_B, rb[set]);
    }
    if (t + 3 < kt) fetch(t + 3, set_c);           // the tile two iterations ahead into the set just emptied
    bx_terms_high<LIVE>(a, b, acc);
    __syncthreads();
  };
  // steady state, as in bxp_loop: no tests, the issue order spelled out (18 LDS stores and 12 dword loads here)
  auto steady = [&](int t, int cur, auto set_c) {
    constexpr int set = decltype(set_c)::value;
    bf16x8_t a[2][3], b[2][3];
    bx_frags<LIVE, PPLANE_A, PPLANE_B, PLD>(As + cur * PBUF_A + aoff, Bs + cur * PBUF_B + boff, 0, a, b);
    bx_terms_low<LIVE>(a, b, acc);
    bxt_store_a(As + (cur ^ 1) * PBUF_A, ra[set]);
    bxt_store_b(Bs + (cur ^ 1) * PBUF_B, rb[set]);
    bxt_load_a<false>(A, lda, m0, kbeg + (t + 3) * PBK, M, kend, ra[set]);
    bxt_load_b<false>(B, ldb, n0, kbeg + (t + 3) * PBK, N, kend, rb[set]);
    bx_terms_high<LIVE>(a, b, acc);
    __builtin_amdgcn_sched_group_barrier(0x100, 12, 0);
#pragma unroll
    for (int g = 0; g < 12; ++g) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x002, 5, 0);
      __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
    }
#pragma unroll
    for (int g = 0; g < 12; ++g) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
    }
    __syncthreads();
  };
  int t = 0;
  if constexpr (LIVE == 15) {
    while (kbeg + (t + 5) * PBK <= kend) {      // two steps per round: tiles t + 3 and t + 4 are read without tests
      steady(t, 0, std::integral_constant<int, 1>{});
      steady(t + 1, 1, std::integral_constant<int, 0>{});
      t += 2;
    }
  }
  // the rest (and edge tiles): the tested step; t is even here, so LDS buffer and register set line up
  for (; t < kt; t += 2) {
    step(t, 0, std::integral_constant<int, 1>{});
    if (t + 1 < kt) step(t + 1, 1, std::integral_constant<int, 0>{});
  }
}

__global__ __launch_bounds__(PTHREADS, 1) void gemm_bxt_kernel(const float* __restrict__ A, const long long lda,
                                                               const float* __restrict__ B, const long long ldb,
                                                               float* __restrict__ C, const int M, const int N, const int K,
                                                               const int k_per_split, const int tiles_n, const int n_tiles) {
  extern __shared__ __attribute__((aligned(16))) unsigned short bxp_lds[];
  unsigned short* As = bxp_lds;
  unsigned short* Bs = bxp_lds + 2 * PBUF_A;
  const int tile = static_cast<int>(blockIdx.x) % n_tiles, z = static_cast<int>(blockIdx.x) / n_tiles;
  const int m0 = (tile / tiles_n) * PBM, n0 = (tile % tiles_n) * BN;
  const int kbeg = z * k_per_split;
  const int kend = (kbeg + k_per_split < K) ? kbeg + k_per_split : K;
  C += static_cast<long long>(z) * M * N;
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  const int li = lane & 31, lk = lane >> 5;
  const WavePlace wp = place_plain(wid, M - m0, N - n0);
  const int wm = wp.wm, wn = wp.wn, live = wp.live;
  f32x16 acc[2][2];
  zero_acc(acc);
  with_live(live, [&](auto live_c) {
    bxt_loop<decltype(live_c)::value>(A, lda, B, ldb, m0, n0, M, N, kbeg, kend, As, Bs, wm, wn, li, lk, acc);
  });
  // partial [M, N] of this K slice: plain stores (splits = 2 selects the epilogue's no-bias, no-activation path)
  gemm_epilogue(acc, m0, n0, wm, wn, li, lk, live, M, N, C, static_cast<long long>(N), nullptr, 0, 2, Epi{}, PBM);
}

// src [rows, cols] f32 (row pitch ld) -> bf16 planes h, m, l in the layout bx6_load_b reads: out[r][c / 8][q][c % 8],
// c < cp = cols rounded up to a multiple of SBK (zero-filled); transpose: out row r is src COLUMN r.
__global__ __launch_bounds__(256) void split_bf16_kernel(const float* __restrict__ src, const long long ld, const int rows,
                                                         const int cols, const int transpose,
                                                         unsigned short* __restrict__ out) {
  const int orows = transpose ? cols : rows, ocols = transpose ? rows : cols;
  const int cp = (ocols + SBK - 1) / SBK * SBK;
  const long long total = static_cast<long long>(orows) * (cp / 2);          // pairs of output elements
  for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < total;
       i += static_cast<long long>(gridDim.x) * blockDim.x) {
    const int r = static_cast<int>(i / (cp / 2)), c = static_cast<int>(i % (cp / 2)) * 2;
    f32x2_t x = {0.f, 0.f};
    if (transpose) {
      if (c < ocols) x[0] = src[static_cast<long long>(c) * ld + r];
      if (c + 1 < ocols) x[1] = src[static_cast<long long>(c + 1) * ld + r];
    } else {
      if (c < ocols) x[0] = src[static_cast<long long>(r) * ld + c];
      if (c + 1 < ocols) x[1] = src[static_cast<long long>(r) * ld + c + 1];
    }
    unsigned h, m, l;
    split2(x, h, m, l);
    unsigned* dst = reinterpret_cast<unsigned*>(out + static_cast<long long>(r) * 3 * cp + (c >> 3) * 24 + (c & 7));
    dst[0] = h;
    dst[4] = m;
    dst[8] = l;
  }
}

}  // namespace rbx
