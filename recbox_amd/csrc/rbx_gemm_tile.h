// rbx_gemm_tile.h -- what the tiled GEMM kernels of rbx_dense.hip share: the output tile a workgroup owns (XCD-aware order),
// the place of a wavefront inside it and which of its 2 x 2 MFMA tiles of 32 x 32 hold any output (`live`), the accumulators,
// and the epilogue with its optional operands.  The k loops are in rbx_gemm_f32.h (f32 MFMAs) and rbx_gemm_bx.h (split
// operands on the bf16 MFMAs); included by rbx_dense.hip.
#pragma once
#include <type_traits>
#include "rbx_internal.h"

namespace rbx {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int BM = 128, BN = 128, BK = 16;
constexpr int kXcds = 8;         // MI355X: 8 accelerator complex dies, 32 CUs and one L2 each
constexpr int LDT = BM + 4;     // LDS row stride (floats): keeps b128 stores aligned, spreads k rows over banks

// Optional tail of the epilogue, applied after bias and activation (all pointers may be NULL):
//   v = mask[row, col] > 0 ? v : 0      ReLU mask taken from ANOTHER tensor (dh = (g W2) o [h > 0]: the activation
//                                       backward of the layer below, without a pass of its own)
//   v += res[row, col]                  residual connection / the second gradient of a tensor with two readers
//   v *= rowscale[row]                  SASRec's timeline mask
// Each of them saves one read-modify-write pass over an [M, N] activation (210 MB at cfg 5).
struct Epi {
  const float* res;
  long long ldres;
  const float* mask;
  long long ldmask;
  const float* rowscale;
  // DeepFM's input block x [M, >= fm_cols] feeds the tower's first GEMM, the FM term and the first-order Linear.  With
  // these set, the dx GEMM of the tower adds the other two readers' gradients to its output columns c < fm_cols:
  //   + fm_g[row] * (fm_s[row, c % fm_dim] - fm_x[row, c])  +  lr_g[row] * lr_w[c]
  // instead of three kernels writing three [M, fm_cols] gradients and a fourth one adding them.
  const float* fm_x;
  long long fm_ldx;
  const float* fm_s;
  const float* fm_g;
  const float* lr_g;
  const float* lr_w;
  int fm_cols;
  int fm_dim;
  int fm_mask;            // fm_dim - 1 when fm_dim is a power of two (col & mask instead of col % dim), else -1
};
__device__ __forceinline__ float epi_fm_term(const Epi& e, int row, int col) {
  if (e.fm_x == nullptr || col >= e.fm_cols) return 0.f;
  const float x = e.fm_x[static_cast<long long>(row) * e.fm_ldx + col];
  const int d = e.fm_mask >= 0 ? (col & e.fm_mask) : (col % e.fm_dim);
  float t = e.fm_g[row] * (e.fm_s[static_cast<long long>(row) * e.fm_dim + d] - x);
  if (e.lr_g != nullptr) t += e.lr_g[row] * e.lr_w[col];
  return t;
}
__device__ __forceinline__ float epi_apply(const Epi& e, float v, int row, int col) {
  if (e.mask != nullptr) v = e.mask[static_cast<long long>(row) * e.ldmask + col] > 0.f ? v : 0.f;
  if (e.res != nullptr) v += e.res[static_cast<long long>(row) * e.ldres + col];
  v += epi_fm_term(e, row, col);
  if (e.rowscale != nullptr) v *= e.rowscale[row];
  return v;
}

// XCD-aware tile order.  Workgroups are dealt round-robin to the 8 XCDs (each with its own 4 MB L2), so launch
// index L runs on XCD L % 8.  Tiles are numbered n-fastest and XCD x works through ONE contiguous range of them:
// the workgroups that share an L2 then share the A row block (all n tiles of an m tile back to back) and walk B in
// the same order, instead of every XCD fetching every A tile.
__device__ __forceinline__ void xcd_tile(const int L, const int tiles_m, const int tiles_n, int* tm_i, int* tn_j) {
  const int total = tiles_m * tiles_n;
  const int xcd = L % kXcds, slot = L / kXcds;
  const int q = total / kXcds, rem = total % kXcds;
  const int tile = xcd * q + (xcd < rem ? xcd : rem) + slot;
  *tm_i = tile / tiles_n;
  *tn_j = tile % tiles_n;
}

// `live`: which of a wavefront's 2 x 2 MFMA tiles hold any output (bit 2 i + j), from the 32-row and 32-column blocks with
// real outputs that lie at and behind its corner.  Valid blocks are a prefix in both directions, so live is 15 (all four),
// 5 (one column of two), 3 (one row of two), 1 or 0.
__device__ __forceinline__ int live_mask(int rows, int cols) {
  rows = rows > 2 ? 2 : rows;
  cols = cols > 2 ? 2 : cols;
  const int live = (rows <= 0 || cols <= 0) ? 0 : (rows == 2 && cols == 2) ? 15 : (rows == 2) ? 5 : (cols == 2) ? 3 : 1;
  return __builtin_amdgcn_readfirstlane(live);
}
// The wavefront's corner inside a 128 x 128 tile of four wavefronts, and its live tiles.  Interior tiles: 2 x 2 wavefronts of
// 64 x 64.  An edge tile with only one or two 32-row (32-column) blocks of real output deals those blocks out over all four
// wavefronts instead of leaving them to one or two of them (M = 400: the last row of tiles has 16 rows -- its wavefronts
// take one 32 x 32 tile each, a quarter of an interior tile's MFMA time, not a half; N = 400: the fourth column tile holds
// 16 columns).  rows_left / cols_left: M - m0, N - n0.
struct WavePlace { int wm, wn, live; };
__device__ __forceinline__ WavePlace place_dealt(const int wid, const int rows_left, const int cols_left) {
  int wm = (wid >> 1) * 64, wn = (wid & 1) * 64;
  const int rb = (rows_left + 31) / 32, cb = (cols_left + 31) / 32;      // blocks with real rows / columns (>= 1)
  int rows, cols;
  if (rb == 1 && cb > 1) { wm = 0; wn = 32 * wid; rows = 1; cols = wid < cb ? 1 : 0; }
  else if (cb == 1 && rb > 1) { wn = 0; wm = 32 * wid; cols = 1; rows = wid < rb ? 1 : 0; }
  else if (rb == 2 && cb > 2) { wm = 32 * (wid & 1); wn = 64 * (wid >> 1); rows = 1; cols = cb - 2 * (wid >> 1); }
  else if (cb == 2 && rb > 2) { wn = 32 * (wid & 1); wm = 64 * (wid >> 1); cols = 1; rows = rb - 2 * (wid >> 1); }
  else { rows = rb - wm / 32; cols = cb - wn / 32; }
  return WavePlace{wm, wn, live_mask(rows, cols)};
}
// The same for a 256 x 128 tile of eight wavefronts: 4 x 2 of 64 x 64, nothing dealt out.
__device__ __forceinline__ WavePlace place_plain(const int wid, const int rows_left, const int cols_left) {
  const int wm = (wid >> 1) * 64, wn = (wid & 1) * 64;
  return WavePlace{wm, wn, live_mask((rows_left - wm + 31) / 32, (cols_left - wn + 31) / 32)};
}

__device__ __forceinline__ void zero_acc(f32x16 (&acc)[2][2]) {
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
}

// f(std::integral_constant<int, live>{}): one copy of a k loop per set of live output tiles (a test per MFMA is two scalar
// instructions beside each of them)
template <class F>
__device__ __forceinline__ void with_live(const int live, F&& f) {
  if (live == 15) f(std::integral_constant<int, 15>{});
  else if (live == 5) f(std::integral_constant<int, 5>{});
  else if (live == 3) f(std::integral_constant<int, 3>{});
  else if (live == 1) f(std::integral_constant<int, 1>{});
  else f(std::integral_constant<int, 0>{});
}

#define RBX_EPI_CH 4   // outputs whose epilogue operands are fetched in one run of loads

// Epilogue of a tile whose wavefronts hold 2 x 2 MFMA tiles of 32 x 32 (C/D layout: col = lane & 31,
// row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5) -- the same for the f32 and the bf16 MFMAs): shared by the tiled kernels.
__device__ __forceinline__ void gemm_epilogue(const f32x16 (&acc)[2][2], const int m0, const int n0, const int wm, const int wn,
                                              const int li, const int lk, const int live, const int M, const int N,
                                              float* __restrict__ C, const long long ldc, const float* __restrict__ bias,
                                              const int act, const int splits, const Epi& epi, const int tile_rows = BM) {
  const bool has_mask = epi.mask != nullptr, has_res = epi.res != nullptr, has_fm = epi.fm_x != nullptr,
             has_lr = epi.lr_g != nullptr, has_rs = epi.rowscale != nullptr;
  if (m0 + tile_rows <= M && n0 + BN <= N && splits == 1 && !(has_fm && (has_mask || has_res || has_rs))) {
    // Interior tile: no row / column tests, and the optional operands of the epilogue are fetched for four outputs at a
    // time in one straight run of loads.  (With a test per output every element was its own basic block -- load, wait,
    // store, 64 times per lane: the DeepFM dx GEMM took 330 us longer than the same GEMM without its epilogue.)
    constexpr int CH = RBX_EPI_CH;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int col = n0 + wn + j * 32 + li;
        const int row0 = m0 + wm + i * 32 + 4 * lk;
        const float bv = bias != nullptr ? bias[col] : 0.f;
#pragma unroll
        for (int h = 0; h < 16; h += CH) {
          float add[CH];
#pragma unroll
          for (int q = 0; q < CH; ++q) add[q] = 0.f;
          if (has_fm) {
            if (col < epi.fm_cols) {
              const int d = epi.fm_mask >= 0 ? (col & epi.fm_mask) : (col % epi.fm_dim);
              const float lw = has_lr ? epi.lr_w[col] : 0.f;
              float x[CH], sm[CH], g[CH], gl[CH];
#pragma unroll
              for (int q = 0; q < CH; ++q) {
                const long long row = row0 + ((h + q) & 3) + 8 * ((h + q) >> 2);
                x[q] = epi.fm_x[row * epi.fm_ldx + col];
                sm[q] = epi.fm_s[row * epi.fm_dim + d];
                g[q] = epi.fm_g[row];
                gl[q] = has_lr ? epi.lr_g[row] : 0.f;
              }
#pragma unroll
              for (int q = 0; q < CH; ++q) add[q] = g[q] * (sm[q] - x[q]) + gl[q] * lw;
            }
#pragma unroll
            for (int q = 0; q < CH; ++q) {
              float v = acc[i][j][h + q] + bv;
              if (act == 1) v = v > 0.f ? v : 0.f;
              C[static_cast<long long>(row0 + ((h + q) & 3) + 8 * ((h + q) >> 2)) * ldc + col] = v + add[q];
            }
          } else {
            float keep[CH], sc[CH];
#pragma unroll
            for (int q = 0; q < CH; ++q) { keep[q] = 1.f; sc[q] = 1.f; }
            if (has_mask) {
#pragma unroll
              for (int q = 0; q < CH; ++q)
                keep[q] = epi.mask[static_cast<long long>(row0 + ((h + q) & 3) + 8 * ((h + q) >> 2)) * epi.ldmask + col];
            }
            if (has_res) {
#pragma unroll
              for (int q = 0; q < CH; ++q)
                add[q] = epi.res[static_cast<long long>(row0 + ((h + q) & 3) + 8 * ((h + q) >> 2)) * epi.ldres + col];
            }
            if (has_rs) {
#pragma unroll
              for (int q = 0; q < CH; ++q) sc[q] = epi.rowscale[row0 + ((h + q) & 3) + 8 * ((h + q) >> 2)];
            }
#pragma unroll
            for (int q = 0; q < CH; ++q) {
              float v = acc[i][j][h + q] + bv;
              if (act == 1) v = v > 0.f ? v : 0.f;
              if (has_mask) v = keep[q] > 0.f ? v : 0.f;
              v += add[q];
              if (has_rs) v *= sc[q];
              C[static_cast<long long>(row0 + ((h + q) & 3) + 8 * ((h + q) >> 2)) * ldc + col] = v;
            }
          }
        }
      }
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = n0 + wn + j * 32 + li;
      if (col >= N || ((live >> (2 * i + j)) & 1) == 0) continue;          // (a tile that is not live may lie over a neighbour's)
      const float bv = (bias != nullptr && splits == 1) ? bias[col] : 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = m0 + wm + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
        if (row < M) {
          float v = acc[i][j][r] + bv;
          if (act == 1 && splits == 1) v = v > 0.f ? v : 0.f;
          if (splits == 1) v = epi_apply(epi, v, row, col);
          C[static_cast<long long>(row) * ldc + col] = v;
        }
      }
    }
  }
}

}  // namespace rbx
