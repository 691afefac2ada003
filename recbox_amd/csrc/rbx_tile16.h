// rbx_tile16.h -- what the kernels built on the 16 x 16 x 4 fp32 MFMA tile (v_mfma_f32_16x16x4_f32, exact fp32) share: the tile
// product over LDS or global operands with its store, and the column sum of the weight-gradient tails.  In all of it a
// wavefront's lane is (col = lane & 15, quad = lane >> 4).  Helpers for every kernel are in rbx_internal.h.
#pragma once
#include "rbx_internal.h"

namespace rbx {

// acc += A B over one 16 x 16 tile: rows m0 .. m0 + 15 of A, columns n0 .. n0 + 15 of B, k < K (a multiple of 4).  A[m][k] lies
// at a[m lda + k] (AT: a[k lda + m]), B[k][n] at b[k ldb + n] (BT: b[n ldb + k]); rows of A from mlim, columns of B from nlim
// and k from klim on count as zeros.  acc[r] is row m0 + 4 quad + r, column n0 + col.  Either operand may lie in LDS or in
// global memory.
//
// The three bounds act as per-lane AND masks on the loaded bits, not as selects: a select keeps its condition in a scalar
// register pair for the whole loop.  Rows from mlim and columns from nlim on are not read: their lanes read row mlim - 1 and
// column nlim - 1 instead, so mlim and nlim must be at least 1.  A k in [klim, K) IS read, at its own address, and masked to +0
// afterwards.  The caller's obligation: with klim < K, every address a[m lda + k] and b[k ldb + n] (in the layout used) with
// m < mlim, n < nlim and klim <= k < K must lie inside the workgroup's LDS, whatever is stored there.  With klim = K nothing
// outside the operands is read.
template <bool AT, bool BT>
__device__ __forceinline__ f32x4 mm16(const float* a, const int lda, const int m0, const int mlim, const float* b, const int ldb,
                                      const int n0, const int nlim, const int K, const int klim, f32x4 acc, const int col,
                                      const int quad) {
  const int mi = m0 + col < mlim ? m0 + col : mlim - 1, ni = n0 + col < nlim ? n0 + col : nlim - 1;
  int amask = m0 + col < mlim ? -1 : 0, bmask = n0 + col < nlim ? -1 : 0;
  asm volatile("" : "+v"(amask), "+v"(bmask));
  const float* ap = AT ? a + quad * lda + mi : a + mi * lda + quad;
  const float* bp = BT ? b + ni * ldb + quad : b + quad * ldb + ni;
  const int as = AT ? 4 * lda : 4, bs = BT ? 4 : 4 * ldb;
  for (int k = quad; k < K; k += 4) {
    const int km = k < klim ? -1 : 0;
    const float av = __int_as_float(__float_as_int(*ap) & amask & km), bv = __int_as_float(__float_as_int(*bp) & bmask & km);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
    ap += as;
    bp += bs;
  }
  return acc;
}

// c[m][n0 + col] = acc's rows m = m0 + 4 quad + r below mlim, for the columns below nlim
__device__ __forceinline__ void store16(float* c, const int ldc, const int m0, const int mlim, const int n0, const int nlim,
                                        const f32x4 acc, const int col, const int quad) {
  if (n0 + col < nlim) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (m0 + 4 * quad + r < mlim) c[(m0 + 4 * quad + r) * ldc + n0 + col] = acc[r];
  }
}

// The sum over the rows of part [rows][row_len] at column e, for a workgroup of 256 threads of which thread tid works on
// e = 16 block + tid % 16 with the row lane r = tid / 16: it adds rows r, r + 16, ... in ascending order, then a halving tree
// over the 16 row lanes runs in sm, which leaves the sum in sm[0][tid % 16].  No column is read from row_len on.
__device__ __forceinline__ void colsum16(const float* part, const int rows, const int row_len, const int e, const int r,
                                         const int c, float (&sm)[16][17]) {
  float s = 0.f;
  if (e < row_len)
    for (int q = r; q < rows; q += 16) s += part[static_cast<long long>(q) * row_len + e];
  sm[r][c] = s;
  __syncthreads();
  for (int o = 8; o > 0; o >>= 1) {
    if (r < o) sm[r][c] += sm[r + o][c];
    __syncthreads();
  }
}

}  // namespace rbx
