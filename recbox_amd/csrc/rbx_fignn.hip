// rbx_fignn.hip -- one message-passing step of FiGNN's field graph (gfx950, wave64): the attentional edge weights, GraphLayer
// and the GRU cell of third_party/recbole/model/context_aware_recommender/fignn.py:119-137 as one launch each way.  Replaces the
// gathered [B, F^2, 2 A] concat in front of Linear(2 A, 1), two broadcast matmuls of [F, A, A] with [B, F, A, 1], a bmm with the
// [B, F, F] graph, nn.GRUCell on [B F, A] (two GEMMs into [B F, 3 A] and an element-wise tail) and the residual add.  Per sample,
// h, h0 [F, A], w_attn [2 A], W_out, W_in [F, A, A], bias_p [A], w_ih, w_hh [3 A, A], b_ih, b_hh [3 A] (gates r, z, n):
//   s_i = w_attn[:A] . h0_i     d_j = w_attn[A:] . h0_j     g[i, :] = softmax_j leaky_relu(s_i + d_j, 0.01), g[i, i] = 0
//   hout_j = W_out[j] h_j       aggr_i = sum_j g[i, j] hout_j        a_i = W_in[i] aggr_i + bias_p
//   r = sig(W_ir a + b_ir + W_hr h + b_hr)   z = sig(W_iz a + b_iz + W_hz h + b_hz)   n = tanh(W_in a + b_in + r (W_hn h + b_hn))
//   h'_i = (1 - z) n + z h_i + h0_i
//
// Geometry.  A workgroup of 1, 2 or 4 wavefronts (as many as the LDS holds) owns a TILE of 16 (at wide shapes 8) samples at a time and walks the
// tiles blockIdx, blockIdx + grid, ...; the grid is min(256, ceil(tiles / 2)).  Two LDS buffers X and Y of [F][16][A + 4] floats
// (row = field * 16 + sample) hold hout and aggr of the tile, so a field's 16 rows are one M tile of samples for the per-field
// matrices and a sample's F rows (stride 16 rows) are the operand of its own F x F products.  The work alternates between
//   per-field phases, a wavefront per field: the tile's h_f staged in the wavefront's scratch, hout_f = h_f W_out[f]^T,
//     a_f = aggr_f W_in[f]^T and the two GRU projections on v_mfma_f32_16x16x4_f32 (exact fp32) with the weight operand read
//     straight from global memory -- every element of W_out[f] and W_in[f] is fetched ONCE per workgroup and tile, by one
//     wavefront, and used for all 16 samples; the gates and the + h0 epilogue stay in the accumulator registers; and
//   per-sample phases, a wavefront per sample: g as an F x F plane in the wavefront's scratch (16 lanes to a row), aggr = g hout
//     on the same MFMA.
// Why 16 samples: the backward needs two [F][16][A + 4] buffers plus scratch, 100 KiB + 42 KiB at 39 fields x 16, which is what
// a compute unit has; a second tile per workgroup would not fit at the shapes that matter, and W_out / W_in (40 .. 160 KiB each)
// stay in the 4 MiB L2 of an XCD, so what a tile re-reads comes from L2, not HBM.  Where even 16 samples do not fit (from 46
// fields at A = 20, 39 at 24, 34 at 28, 30 at 32; 39 x 32 is one of them) a tile is 8 samples: the buffers are [F][8][A + 4], the
// upper 8 rows of the per-field MFMA tiles are masked to zero, and a field's matrix serves 8 samples per fetch.
// The cell's weights w_ih, w_hh (6 A^2 floats, shared by all fields) are NOT staged: every field of every tile reads them as
// MFMA operands straight from global memory, 24 .. 96 KiB that stay in L1 / L2.  The registers that rbx_gru.hip gives to W_hh hold
// dw_ih and dw_hh here, and LDS has no room left at the large shapes; staging them per workgroup is what a measurement of the
// small shapes would have to justify.  No F^2-by-A tensor exists anywhere.
//
// fignn_step_fwd_kernel   writes h' [B, F, A] and, when asked, g [B, F, F].
// fignn_step_bwd_kernel   saves nothing: recomputes s, d, g, hout, aggr, a and the gates, then per field dgi, dgh, da = dgi W_ih,
//                         dh = dy z + dgh W_hh, daggr = da W_in[f] (into Y in place of aggr); per sample dg = daggr hout^T, the
//                         softmax and leaky-relu backward, ds, dd and dhout = g^T daggr (into X in place of hout); per field
//                         dh += dhout W_out[f], dh0 = dy + ds w_s + dd w_d.  dw_ih, dw_hh stay in MFMA accumulators and the
//                         bias / w_attn sums in registers over all tiles of a wavefront: one row per wavefront in the
//                         workspace's second part.  dW_out[f] and dW_in[f] belong to a field, not to a wavefront, so they are
//                         added tile after tile into the workgroup's own row of the workspace's first part (always by the same
//                         lane, so no synchronisation).  fignn_tail_kernel adds the rows of both parts in a fixed order.
// Workspace: grid x 2 F A^2 + grid x waves x (6 A^2 + 9 A) floats, grid <= 256: at most 26 MiB at 39 x 16, 91 MiB at 39 x 32.
// No atomics, every sum in a fixed order: two runs give the same bits.  No host read-back, nothing allocated, everything on the
// caller's stream.  Every index is bounded by batch, n_fields and dim.
#include "rbx_internal.h"
#include "rbx_tile16.h"

namespace rbx {

constexpr int kFgMinF = 2, kFgMaxF = 48;    // the softmax walks a row in three chunks of 16 lanes
constexpr int kFgMinA = 4, kFgMaxA = 32;    // dw_ih and dw_hh [3 A, A] are held in 24 NE^2 accumulator registers
constexpr int kFgTile = 16;                 // samples of a tile: the M of one MFMA
constexpr int kFgMaxGrid = 256;             // workgroups of a launch = rows of the workspace's first part
constexpr size_t kFgLdsCap = 160 * 1024;    // LDS of a gfx950 compute unit
constexpr float kFgSlope = 0.01f;           // nn.LeakyReLU(negative_slope=0.01)

struct FgArgs {
  const float* h;        // [B, F, A]
  const float* h0;       // [B, F, A]
  const float* wattn;    // [2 A]
  const float* wout;     // [F, A, A]
  const float* win;      // [F, A, A]
  const float* biasp;    // [A]
  const float* wih;      // [3 A, A]
  const float* whh;      // [3 A, A]
  const float* bih;      // [3 A]
  const float* bhh;      // [3 A]
  const float* dy;       // backward: [B, F, A]
  float* y;              // forward: [B, F, A]
  float* graph;          // forward: [B, F, F] or NULL
  float* dh;             // backward: [B, F, A] or NULL
  float* dh0;            // backward: [B, F, A] or NULL
  float* part1;          // backward: [grid][2 F A A] (dW_out | dW_in) or NULL (no weight gradient wanted)
  float* part2;          // backward: [grid waves][6 A A + 9 A] (dw_ih | dw_hh | db_ih | db_hh | dbias_p | dw_attn)
  long long B;
  int F, A, T, tshift;   // T = 1 << tshift: the samples of a tile, 16 or 8
};

// (its own name for pad16 of rbx_internal.h: tests/test_gpu_fignn_forms.py holds the layout lines below to their text)
static __host__ __device__ inline int fg_pad16(int n) { return pad16(n); }
static __host__ __device__ inline int fg_row1(int F, int A) { return 2 * F * A * A; }
static __host__ __device__ inline int fg_row2(int A) { return 6 * A * A + 9 * A; }
// a wavefront's scratch: the forward stages h_f and a_f [16][A + 4]; the backward adds da_f and dgi, dgh [16][3 A + 4]; both
// share it with the g plane [pad16(F)][pad16(F) + 4]
static __host__ __device__ inline int fg_scratch(int F, int A, bool bwd) {
  const int FP = fg_pad16(F), plane = FP * (FP + 4);
  const int field = bwd ? kFgTile * (3 * (A + 4) + 2 * (3 * A + 4)) : kFgTile * 2 * (A + 4);
  return plane > field ? plane : field;
}
// X, Y [F][16][A + 4]; s, d, ds, dd [F][16]
static __host__ __device__ inline int fg_shared(int F, int A, int T) { return 2 * F * T * (A + 4) + 4 * F * T; }
static size_t fg_lds(int F, int A, bool bwd, int nw, int T) {
  return 4 * (static_cast<size_t>(fg_shared(F, A, T)) + static_cast<size_t>(nw) * fg_scratch(F, A, bwd));
}
// 16 samples to a tile where the backward's LDS holds that, else 8 (the upper 8 rows of the per-field MFMA tiles are then zeros)
static int fg_tile(int F, int A) { return fg_lds(F, A, true, 1, kFgTile) <= kFgLdsCap ? kFgTile : kFgTile / 2; }
static int fg_waves(int F, int A, bool bwd) {
  const int T = fg_tile(F, A);
  for (int nw = 4; nw > 1; nw >>= 1)
    if (fg_lds(F, A, bwd, nw, T) <= kFgLdsCap) return nw;
  return 1;
}
// every workgroup takes at least two tiles where the batch has them: half the workspace rows for the same work
static unsigned fg_grid(int64_t batch, int T) {
  const int64_t tiles = (batch + T - 1) / T, need = (tiles + 1) / 2;
  return static_cast<unsigned>(need < kFgMaxGrid ? need : kFgMaxGrid);
}

// the sum over the four lanes that hold one column of an accumulator tile
__device__ __forceinline__ float fg_sumq(float v) {
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}

// The products are mm16 / store16 of rbx_tile16.h, whose klim < K reads past the operand and asks the caller to show that those
// addresses are LDS of the workgroup.  Here only LDS operands are called with klim < K, and a k from klim on reads up to 3 field
// rows past a sample's plane or slab (K = pad4(F), klim = F), or, on 8-sample tiles, the 8 rows behind a field's slab (K = 16,
// klim = 8), which for the last field are the start of Y, or of s, d and the scratch.  Those addresses lie inside the
// workgroup's LDS: 8-sample tiles occur only from 30 fields on, where the 4 F T floats of s, d, ds, dd alone exceed 8 rows of
// A + 4; and 3 T rows past Y (K = pad4(F)) are fewer floats than s .. dd plus the wavefronts' scratch (four times at least
// 16 x 2 (A + 4) at the small F where s .. dd are short).

// the tile's rows of field f, src[(b0 + s) F + f][..], s < 16, into dst [16][A + 4]; zeros for samples from nb on
__device__ __forceinline__ void fg_stage(const float* src, const long long b0, const int nb, const int f, const int F, const int A,
                                         const int lane, float* dst) {
  const int a4 = A >> 2, ld = A + 4;
  for (int idx = lane; idx < kFgTile * a4; idx += 64) {
    const int s = idx / a4, q = idx - s * a4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (s < nb) v = *reinterpret_cast<const float4*>(src + ((b0 + s) * F + f) * A + 4 * q);
    *reinterpret_cast<float4*>(dst + s * ld + 4 * q) = v;
  }
}

// s and d of every (field, sample) of the tile into sv, dv [F][16]; zeros for samples from nb on.  The whole workgroup.
__device__ __forceinline__ void fg_edges(const FgArgs& g, const long long b0, const int nb, float* sv, float* dv) {
  const int F = g.F, A = g.A;
  for (int r = threadIdx.x; r < F * g.T; r += blockDim.x) {
    const int f = r >> g.tshift, s = r & (g.T - 1);
    float ss = 0.f, dd = 0.f;
    if (s < nb) {
      const float* p = g.h0 + ((b0 + s) * F + f) * A;
      for (int e = 0; e < A; e += 4) {
        const float4 v = *reinterpret_cast<const float4*>(p + e);
        const float4 ws = *reinterpret_cast<const float4*>(g.wattn + e);
        const float4 wd = *reinterpret_cast<const float4*>(g.wattn + A + e);
        ss += v.x * ws.x + v.y * ws.y + v.z * ws.z + v.w * ws.w;
        dd += v.x * wd.x + v.y * wd.y + v.z * wd.z + v.w * wd.w;
      }
    }
    sv[r] = ss;
    dv[r] = dd;
  }
}

// g of sample s as a plane pl [i][j], i, j < F at row stride pad16(F) + 4: four rows at a time, 16 lanes to a row; to graph
// when not NULL.  Forward and backward call this.
__device__ __forceinline__ void fg_plane(const float* sv, const float* dv, const int s, const int F, const int T, float* pl, float* graph,
                                         const int col, const int quad) {
  const int FP = fg_pad16(F), ldp = FP + 4;
  for (int i = quad; i < FP; i += 4) {       // uniform over the wavefront: the shuffles see every lane
    const float si = i < F ? sv[i * T + s] : 0.f;
    float e[3], m = -INFINITY;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int j = col + 16 * c;
      float al = -INFINITY;
      if (j < F && j != i) {
        al = si + dv[j * T + s];
        al = al > 0.f ? al : kFgSlope * al;
      }
      e[c] = al;
      m = fmaxf(m, al);
    }
    m = group_max<16, kWave>(m);
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      e[c] = e[c] > -INFINITY ? expf(e[c] - m) : 0.f;
      sum += e[c];
    }
    sum = group_sum<16, kWave>(sum);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int j = col + 16 * c;
      if (i < F && j < F) {
        const float p = e[c] / sum;
        pl[i * ldp + j] = p;
        if (graph != nullptr) graph[i * F + j] = p;
      }
    }
  }
}

// The base pointers as per-lane values.  Seventeen uniform pointers and what the compiler derives from them do not fit in the
// scalar registers beside the loop state (it then parks scalars in vector lanes); every use adds a per-lane index anyway.
template <typename T>
__device__ __forceinline__ T* fg_v(T* p) {
  asm volatile("" : "+v"(p));
  return p;
}
__device__ __forceinline__ FgArgs fg_in_vgprs(const FgArgs& a) {
  FgArgs g = a;
  g.h = fg_v(a.h); g.h0 = fg_v(a.h0); g.wattn = fg_v(a.wattn); g.wout = fg_v(a.wout); g.win = fg_v(a.win);
  g.biasp = fg_v(a.biasp); g.wih = fg_v(a.wih); g.whh = fg_v(a.whh); g.bih = fg_v(a.bih); g.bhh = fg_v(a.bhh);
  g.dy = fg_v(a.dy); g.y = fg_v(a.y); g.graph = fg_v(a.graph); g.dh = fg_v(a.dh); g.dh0 = fg_v(a.dh0);
  g.part1 = fg_v(a.part1); g.part2 = fg_v(a.part2);
  return g;
}

extern __shared__ __attribute__((aligned(16))) float fg_smem[];

// X = hout of the tile: a wavefront per field.  Ends with a barrier.
__device__ __forceinline__ void fg_hout(const FgArgs& g, const long long b0, const int nb, float* X, float* th, const int wv,
                                        const int nw, const int lane, const int col, const int quad) {
  const int F = g.F, A = g.A, ld = A + 4;
  for (int f0 = 0; f0 < F; f0 += nw) {       // uniform over the workgroup
    const int f = f0 + wv;
    const bool ok = f < F;
    if (ok) fg_stage(g.h, b0, nb, f, F, A, lane, th);
    __syncthreads();
    if (ok)
      for (int nt = 0; 16 * nt < A; ++nt)
        store16(X + f * g.T * ld, ld, 0, g.T, 16 * nt, A,
                 mm16<false, true>(th, ld, 0, kFgTile, g.wout + f * A * A, A, 16 * nt, A, A, A, f32x4{0.f, 0.f, 0.f, 0.f}, col, quad),
                 col, quad);
    __syncthreads();
  }
}

// Y = aggr of the tile from X = hout: a wavefront per sample, g in its scratch.  Ends with a barrier.
__device__ __forceinline__ void fg_aggr(const FgArgs& g, const long long b0, const int nb, const float* X, float* Y, const float* sv,
                                        const float* dv, float* pl, const bool graph, const int wv, const int nw, const int col,
                                        const int quad) {
  const int F = g.F, A = g.A, ld = A + 4, ldp = fg_pad16(F) + 4, K = (F + 3) & ~3;
  for (int s0 = 0; s0 < g.T; s0 += nw) { // uniform: nw divides the tile
    const int s = s0 + wv;
    fg_plane(sv, dv, s, F, g.T, pl, (graph && g.graph != nullptr && s < nb) ? g.graph + (b0 + s) * F * F : nullptr, col, quad);
    __syncthreads();
    for (int mt = 0; 16 * mt < F; ++mt)
      for (int nt = 0; 16 * nt < A; ++nt)
        store16(Y + s * ld, g.T * ld, 16 * mt, F, 16 * nt, A,
                 mm16<false, false>(pl, ldp, 16 * mt, F, X + s * ld, g.T * ld, 16 * nt, A, K, F, f32x4{0.f, 0.f, 0.f, 0.f}, col,
                                     quad),
                 col, quad);
    __syncthreads();
  }
}

// The kernels' view of their arguments and of the LDS, made AFRESH at the head of every loop body: F, A and T pass through an
// empty volatile asm there, so nothing derived from them (strides, LDS addresses, per-field offsets) is hoisted out of that
// body and kept in a scalar register across the other phases.  Hoisted, that state needs more than the 106 SGPRs there are;
// recomputed, it is a few scalar instructions per field or sample.
#define FG_FRESH_COMMON                                                                                                      \
  FgArgs g = gk;                                                                                                             \
  asm volatile("" : "+s"(g.F), "+s"(g.A), "+s"(g.T));                                                                        \
  __attribute__((unused)) const int F = g.F, A = g.A, ld = A + 4, R = F * g.T;                                               \
  __attribute__((unused)) float* const X = fg_smem;                                                                          \
  __attribute__((unused)) float* const Y = X + R * ld;                                                                       \
  __attribute__((unused)) float* const sv = Y + R * ld;                                                                      \
  __attribute__((unused)) float* const dv = sv + R
#define FG_FWD_FRESH                                                                                                         \
  FG_FRESH_COMMON;                                                                                                           \
  __attribute__((unused)) float* const scr = fg_smem + fg_shared(F, A, g.T) + wv * fg_scratch(F, A, false);                  \
  __attribute__((unused)) float* const th = scr;                                                                             \
  __attribute__((unused)) float* const ta = scr + kFgTile * ld
#define FG_BWD_FRESH                                                                                                         \
  FG_FRESH_COMMON;                                                                                                           \
  __attribute__((unused)) const int A3 = 3 * A, ld3 = A3 + 4, ldp = fg_pad16(F) + 4, KF = (F + 3) & ~3;                      \
  __attribute__((unused)) float* const dsv = dv + R;                                                                         \
  __attribute__((unused)) float* const ddv = dsv + R;                                                                        \
  __attribute__((unused)) float* const scr = fg_smem + fg_shared(F, A, g.T) + wv * fg_scratch(F, A, true);                   \
  __attribute__((unused)) float* const th = scr;                                                                             \
  __attribute__((unused)) float* const ta = th + kFgTile * ld;                                                               \
  __attribute__((unused)) float* const tda = ta + kFgTile * ld;                                                              \
  __attribute__((unused)) float* const dgi = tda + kFgTile * ld;                                                             \
  __attribute__((unused)) float* const dgh = dgi + kFgTile * ld3

template <int NE>
__global__ __launch_bounds__(256) void fignn_step_fwd_kernel(const FgArgs ga) {
  const FgArgs gk = fg_in_vgprs(ga);
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), col = lane & 15, quad = lane >> 4, nw = blockDim.x >> 6;
  const long long tiles = (ga.B + ga.T - 1) >> ga.tshift;

  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {                     // uniform over the workgroup
    FG_FWD_FRESH;
    const long long b0 = tile * g.T;
    const int nb = g.B - b0 < g.T ? static_cast<int>(g.B - b0) : g.T;
    fg_edges(g, b0, nb, sv, dv);
    fg_hout(g, b0, nb, X, th, wv, nw, lane, col, quad);
    fg_aggr(g, b0, nb, X, Y, sv, dv, scr, true, wv, nw, col, quad);

    for (int f0 = 0; f0 < F; f0 += nw) {
      FG_FWD_FRESH;
      const int f = f0 + wv;
      const bool ok = f < F;
      if (ok) {
        fg_stage(g.h, b0, nb, f, F, A, lane, th);
#pragma unroll
        for (int nt = 0; nt < NE; ++nt) {
          if (16 * nt < A) {
            const int n = 16 * nt + col;
            f32x4 acc = mm16<false, true>(Y + f * g.T * ld, ld, 0, g.T, g.win + f * A * A, A, 16 * nt, A, A, A,
                                              f32x4{0.f, 0.f, 0.f, 0.f}, col, quad);
            const float bp = n < A ? g.biasp[n] : 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[r] += bp;
            store16(ta, ld, 0, kFgTile, 16 * nt, A, acc, col, quad);
          }
        }
      }
      __syncthreads();
      if (ok) {
#pragma unroll
        for (int nt = 0; nt < NE; ++nt) {
          if (16 * nt < A) {
            const int n = 16 * nt + col;
            f32x4 gi[3], gh[3];
#pragma unroll
            for (int q = 0; q < 3; ++q) {
              gi[q] = mm16<false, true>(ta, ld, 0, kFgTile, g.wih + q * A * A, A, 16 * nt, A, A, A, f32x4{0.f, 0.f, 0.f, 0.f}, col, quad);
              gh[q] = mm16<false, true>(th, ld, 0, kFgTile, g.whh + q * A * A, A, 16 * nt, A, A, A, f32x4{0.f, 0.f, 0.f, 0.f}, col, quad);
            }
            if (n < A) {
              float bi[3], bh[3];
#pragma unroll
              for (int q = 0; q < 3; ++q) {
                bi[q] = g.bih[q * A + n];
                bh[q] = g.bhh[q * A + n];
              }
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const int s = 4 * quad + r;
                if (s < nb) {
                  const float rg = sigmoidf_fast(gi[0][r] + bi[0] + gh[0][r] + bh[0]);
                  const float zg = sigmoidf_fast(gi[1][r] + bi[1] + gh[1][r] + bh[1]);
                  const float ng = tanhf_fast(gi[2][r] + bi[2] + rg * (gh[2][r] + bh[2]));
                  const long long at = ((b0 + s) * F + f) * A + n;
                  g.y[at] = (1.f - zg) * ng + zg * th[s * ld + n] + g.h0[at];
                }
              }
            }
          }
        }
      }
      __syncthreads();                       // th and ta are written again
    }
  }
}

template <int NE>
__global__ __launch_bounds__(256) void fignn_step_bwd_kernel(const FgArgs ga) {
  const FgArgs gk = fg_in_vgprs(ga);
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), col = lane & 15, quad = lane >> 4, nw = blockDim.x >> 6;
  const bool want_w = ga.part1 != nullptr;
  const long long tiles = (ga.B + ga.T - 1) >> ga.tshift;
  const f32x4 zero = f32x4{0.f, 0.f, 0.f, 0.f};

  f32x4 dwih[3 * NE][NE], dwhh[3 * NE][NE];     // [16 m + 4 quad + r][16 n + col] over this wavefront's fields and tiles
  float dbi[3][NE], dbn[NE], dbp[NE], dws[NE], dwd[NE];   // column 16 n + col: db_ih, the n gate of db_hh, dbias_p, dw_attn
#pragma unroll
  for (int n = 0; n < NE; ++n) {
#pragma unroll
    for (int m = 0; m < 3 * NE; ++m) {
      dwih[m][n] = zero;
      dwhh[m][n] = zero;
    }
    dbi[0][n] = dbi[1][n] = dbi[2][n] = dbn[n] = dbp[n] = dws[n] = dwd[n] = 0.f;
  }

  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {                     // uniform over the workgroup
    FG_BWD_FRESH;
    const long long b0 = tile * g.T;
    const int nb = g.B - b0 < g.T ? static_cast<int>(g.B - b0) : g.T;
    const bool first = tile == blockIdx.x;
    fg_edges(g, b0, nb, sv, dv);
    fg_hout(g, b0, nb, X, th, wv, nw, lane, col, quad);
    fg_aggr(g, b0, nb, X, Y, sv, dv, scr, false, wv, nw, col, quad);

    // per field: the cell again and its backward; Y_f turns from aggr_f into daggr_f
    for (int f0 = 0; f0 < F; f0 += nw) {
      FG_BWD_FRESH;
      const int f = f0 + wv;
      const bool ok = f < F;
      float* Yf = Y + f * g.T * ld;
      if (ok) {
        fg_stage(g.h, b0, nb, f, F, A, lane, th);
#pragma unroll
        for (int nt = 0; nt < NE; ++nt) {
          if (16 * nt < A) {
            const int n = 16 * nt + col;
            f32x4 acc = mm16<false, true>(Yf, ld, 0, g.T, g.win + f * A * A, A, 16 * nt, A, A, A, zero, col, quad);
            const float bp = n < A ? g.biasp[n] : 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[r] += bp;
            store16(ta, ld, 0, kFgTile, 16 * nt, A, acc, col, quad);
          }
        }
      }
      __syncthreads();
      f32x4 dhp[NE];                      // dy z: the part of dh that does not pass the cell's matrices
      if (ok) {
#pragma unroll
        for (int nt = 0; nt < NE; ++nt) {
          dhp[nt] = zero;
          if (16 * nt < A) {
            const int n = 16 * nt + col;
            f32x4 gi[3], gh[3];
#pragma unroll
            for (int q = 0; q < 3; ++q) {
              gi[q] = mm16<false, true>(ta, ld, 0, kFgTile, g.wih + q * A * A, A, 16 * nt, A, A, A, zero, col, quad);
              gh[q] = mm16<false, true>(th, ld, 0, kFgTile, g.whh + q * A * A, A, 16 * nt, A, A, A, zero, col, quad);
            }
            if (n < A) {
              float bi[3], bh[3];
#pragma unroll
              for (int q = 0; q < 3; ++q) {
                bi[q] = g.bih[q * A + n];
                bh[q] = g.bhh[q * A + n];
              }
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const int s = 4 * quad + r;
                const float dyv = s < nb ? g.dy[((b0 + s) * F + f) * A + n] : 0.f;
                const float ghn = gh[2][r] + bh[2];
                const float rg = sigmoidf_fast(gi[0][r] + bi[0] + gh[0][r] + bh[0]);
                const float zg = sigmoidf_fast(gi[1][r] + bi[1] + gh[1][r] + bh[1]);
                const float ng = tanhf_fast(gi[2][r] + bi[2] + rg * ghn);
                const float dnp = dyv * (1.f - zg) * (1.f - ng * ng);
                const float dzp = dyv * (th[s * ld + n] - ng) * zg * (1.f - zg);
                const float drp = dnp * ghn * rg * (1.f - rg);
                dgi[s * ld3 + n] = drp;
                dgi[s * ld3 + A + n] = dzp;
                dgi[s * ld3 + 2 * A + n] = dnp;
                dgh[s * ld3 + n] = drp;
                dgh[s * ld3 + A + n] = dzp;
                dgh[s * ld3 + 2 * A + n] = dnp * rg;
                dhp[nt][r] = dyv * zg;
                dbi[0][nt] += drp;
                dbi[1][nt] += dzp;
                dbi[2][nt] += dnp;
                dbn[nt] += dnp * rg;
              }
            }
          }
        }
      }
      __syncthreads();                       // dgi, dgh
      if (ok) {
#pragma unroll
        for (int nt = 0; nt < NE; ++nt) {
          if (16 * nt < A) {
            const int n = 16 * nt + col;
            const f32x4 da = mm16<false, false>(dgi, ld3, 0, kFgTile, g.wih, A, 16 * nt, A, A3, A3, zero, col, quad);
            store16(tda, ld, 0, kFgTile, 16 * nt, A, da, col, quad);
            dbp[nt] += (da[0] + da[1]) + (da[2] + da[3]);
            if (g.dh != nullptr) {
              const f32x4 d = mm16<false, false>(dgh, ld3, 0, kFgTile, g.whh, A, 16 * nt, A, A3, A3, dhp[nt], col, quad);
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const int s = 4 * quad + r;
                if (s < nb && n < A) g.dh[((b0 + s) * F + f) * A + n] = d[r];
              }
            }
            if (want_w) {
#pragma unroll
              for (int m = 0; m < 3 * NE; ++m)
                if (16 * m < A3) {
                  dwih[m][nt] = mm16<true, false>(dgi, ld3, 16 * m, A3, ta, ld, 16 * nt, A, kFgTile, kFgTile, dwih[m][nt], col, quad);
                  dwhh[m][nt] = mm16<true, false>(dgh, ld3, 16 * m, A3, th, ld, 16 * nt, A, kFgTile, kFgTile, dwhh[m][nt], col, quad);
                }
            }
          }
        }
      }
      __syncthreads();                       // da_f
      f32x4 dag[NE];
      if (ok) {
#pragma unroll
        for (int nt = 0; nt < NE; ++nt) {
          dag[nt] = zero;
          if (16 * nt < A) {
            if (want_w) {                    // dW_in[f] += da_f^T aggr_f, into the workgroup's row
              float* dst = g.part1 + static_cast<long long>(blockIdx.x) * fg_row1(F, A) + (F + f) * A * A;
#pragma unroll
              for (int mt = 0; mt < NE; ++mt)
                if (16 * mt < A) {
                  const f32x4 w = mm16<true, false>(tda, ld, 16 * mt, A, Yf, ld, 16 * nt, A, kFgTile, g.T, zero, col, quad);
#pragma unroll
                  for (int r = 0; r < 4; ++r) {
                    const int m = 16 * mt + 4 * quad + r, n = 16 * nt + col;
                    if (m < A && n < A) dst[m * A + n] = first ? w[r] : dst[m * A + n] + w[r];
                  }
                }
            }
            dag[nt] = mm16<false, false>(tda, ld, 0, kFgTile, g.win + f * A * A, A, 16 * nt, A, A, A, zero, col, quad);
          }
        }
      }
      __syncthreads();                       // aggr_f is read
      if (ok) {
#pragma unroll
        for (int nt = 0; nt < NE; ++nt)
          if (16 * nt < A) store16(Yf, ld, 0, g.T, 16 * nt, A, dag[nt], col, quad);
      }
      __syncthreads();                       // the scratch is written again; after the last field: Y = daggr
    }

    // per sample: dg = daggr hout^T, through the softmax and the leaky relu to ds and dd; X_s turns from hout into dhout = g^T daggr
    for (int s0 = 0; s0 < g.T; s0 += nw) {
      FG_BWD_FRESH;
      const int s = s0 + wv;
      const float* Ys = Y + s * ld;
      float* Xs = X + s * ld;
      fg_plane(sv, dv, s, F, g.T, scr, nullptr, col, quad);
      __syncthreads();
      float cd[3] = {0.f, 0.f, 0.f};         // dd of the columns col + 16 c
      for (int mt = 0; 16 * mt < F; ++mt) {
        f32x4 dg[3];
        float p[3][4], rs[4] = {0.f, 0.f, 0.f, 0.f}, dsr[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          dg[c] = zero;
          if (16 * c < F) dg[c] = mm16<false, true>(Ys, g.T * ld, 16 * mt, F, Xs, g.T * ld, 16 * c, F, A, A, zero, col, quad);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int i = 16 * mt + 4 * quad + r, j = 16 * c + col;
            p[c][r] = (i < F && j < F && i != j) ? scr[i * ldp + j] : 0.f;
            rs[r] += p[c][r] * dg[c][r];
          }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) rs[r] = group_sum<16, kWave>(rs[r]);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int i = 16 * mt + 4 * quad + r, j = 16 * c + col;
            float da = p[c][r] * (dg[c][r] - rs[r]);
            if (i < F && j < F && !(sv[i * g.T + s] + dv[j * g.T + s] > 0.f)) da *= kFgSlope;
            dsr[r] += da;
            cd[c] += da;
          }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = 16 * mt + 4 * quad + r;
          const float t = group_sum<16, kWave>(dsr[r]);
          if (col == 0 && i < F) dsv[i * g.T + s] = t;
        }
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float t = fg_sumq(cd[c]);
        if (quad == 0 && 16 * c + col < F) ddv[(16 * c + col) * g.T + s] = t;
      }
      __syncthreads();                       // hout of the sample is read
      for (int mt = 0; 16 * mt < F; ++mt)
        for (int nt = 0; 16 * nt < A; ++nt)
          store16(Xs, g.T * ld, 16 * mt, F, 16 * nt, A,
                   mm16<true, false>(scr, ldp, 16 * mt, F, Ys, g.T * ld, 16 * nt, A, KF, F, zero, col, quad), col, quad);
      __syncthreads();                       // the plane is written again; after the last sample: X = dhout, ds, dd
    }

    // per field: dW_out[f] += dhout_f^T h_f, dh_f += dhout_f W_out[f], dh0_f = dy_f + ds w_s + dd w_d, dw_attn
    for (int f0 = 0; f0 < F; f0 += nw) {
      FG_BWD_FRESH;
      const int f = f0 + wv;
      const bool ok = f < F;
      const float* Xf = X + f * g.T * ld;
      if (ok && want_w) fg_stage(g.h, b0, nb, f, F, A, lane, th);
      __syncthreads();
      if (ok) {
#pragma unroll
        for (int nt = 0; nt < NE; ++nt) {
          if (16 * nt < A) {
            const int n = 16 * nt + col;
            if (want_w) {
              float* dst = g.part1 + static_cast<long long>(blockIdx.x) * fg_row1(F, A) + f * A * A;
#pragma unroll
              for (int mt = 0; mt < NE; ++mt)
                if (16 * mt < A) {
                  const f32x4 w = mm16<true, false>(Xf, ld, 16 * mt, A, th, ld, 16 * nt, A, kFgTile, g.T, zero, col, quad);
#pragma unroll
                  for (int r = 0; r < 4; ++r) {
                    const int m = 16 * mt + 4 * quad + r;
                    if (m < A && n < A) dst[m * A + n] = first ? w[r] : dst[m * A + n] + w[r];
                  }
                }
            }
            f32x4 d = zero;
            if (g.dh != nullptr) d = mm16<false, false>(Xf, ld, 0, g.T, g.wout + f * A * A, A, 16 * nt, A, A, A, zero, col, quad);
            if (n < A) {
              const float ws = g.wattn[n], wd = g.wattn[A + n];
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const int s = 4 * quad + r;
                if (s < nb) {
                  const long long at = ((b0 + s) * F + f) * A + n;
                  const float dsi = dsv[f * g.T + s], ddi = ddv[f * g.T + s];
                  if (g.dh != nullptr) g.dh[at] += d[r];               // what this lane wrote in the cell's phase
                  if (g.dh0 != nullptr) g.dh0[at] = g.dy[at] + dsi * ws + ddi * wd;
                  if (want_w) {
                    const float h0v = g.h0[at];
                    dws[nt] += dsi * h0v;
                    dwd[nt] += ddi * h0v;
                  }
                }
              }
            }
          }
        }
      }
      __syncthreads();                       // th is written again; the next tile writes X, Y, s and d
    }
  }

  if (want_w) {                              // this wavefront's row of the second part
    FG_BWD_FRESH;
    float* row = g.part2 + (static_cast<long long>(blockIdx.x) * nw + wv) * fg_row2(A);
    float* rhh = row + A3 * A;
    float* rb = rhh + A3 * A;                // db_ih [3 A] | db_hh [3 A] | dbias_p [A] | dw_attn [2 A]
#pragma unroll
    for (int nt = 0; nt < NE; ++nt) {
      const int n = 16 * nt + col;
#pragma unroll
      for (int m = 0; m < 3 * NE; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int u = 16 * m + 4 * quad + r;
          if (u < A3 && n < A) {
            row[u * A + n] = dwih[m][nt][r];
            rhh[u * A + n] = dwhh[m][nt][r];
          }
        }
      const float t0 = fg_sumq(dbi[0][nt]), t1 = fg_sumq(dbi[1][nt]), t2 = fg_sumq(dbi[2][nt]), t3 = fg_sumq(dbn[nt]);
      const float t4 = fg_sumq(dbp[nt]), t5 = fg_sumq(dws[nt]), t6 = fg_sumq(dwd[nt]);
      if (quad == 0 && n < A) {
        rb[n] = t0;
        rb[A + n] = t1;
        rb[2 * A + n] = t2;
        rb[A3 + n] = t0;
        rb[A3 + A + n] = t1;
        rb[A3 + 2 * A + n] = t3;
        rb[2 * A3 + n] = t4;
        rb[2 * A3 + A + n] = t5;
        rb[2 * A3 + 2 * A + n] = t6;
      }
    }
  }
}

struct FgTail {
  const float* part1;
  const float* part2;
  int rows1, rows2, len1, len2, blocks1;
  int F, A;
  float* dst[8];         // dW_out, dW_in | dw_ih, dw_hh, db_ih, db_hh, dbias_p, dw_attn; NULL: skipped
};

// out[e] = the sum over the rows of one part of the workspace: thread (row lane r = tid / 16, column tid % 16) adds rows r,
// r + 16, ... in ascending order, then a tree over the 16 row lanes.  Blocks below blocks1 take the first part, the others the
// second.
__global__ __launch_bounds__(256) void fignn_tail_kernel(const FgTail t) {
  __shared__ float sm[16][17];
  const bool one = static_cast<int>(blockIdx.x) < t.blocks1;
  const float* part = one ? t.part1 : t.part2;
  const int rows = one ? t.rows1 : t.rows2, rl = one ? t.len1 : t.len2;
  const int c = threadIdx.x & 15, r = threadIdx.x >> 4, e = ((one ? blockIdx.x : blockIdx.x - t.blocks1) * 16) + c;
  float s = 0.f;
  if (e < rl)
    for (int q = r; q < rows; q += 16) s += part[static_cast<long long>(q) * rl + e];
  sm[r][c] = s;
  __syncthreads();
  for (int o = 8; o > 0; o >>= 1) {
    if (r < o) sm[r][c] += sm[r + o][c];
    __syncthreads();
  }
  if (r == 0 && e < rl) {
    const int A = t.A, faa = t.F * A * A, a3a = 3 * A * A;
    float* dst;
    int at;
    if (one) {
      dst = e < faa ? t.dst[0] : t.dst[1];
      at = e < faa ? e : e - faa;
    } else if (e < a3a) {
      dst = t.dst[2]; at = e;
    } else if (e < 2 * a3a) {
      dst = t.dst[3]; at = e - a3a;
    } else if (e < 2 * a3a + 3 * A) {
      dst = t.dst[4]; at = e - 2 * a3a;
    } else if (e < 2 * a3a + 6 * A) {
      dst = t.dst[5]; at = e - 2 * a3a - 3 * A;
    } else if (e < 2 * a3a + 7 * A) {
      dst = t.dst[6]; at = e - 2 * a3a - 6 * A;
    } else {
      dst = t.dst[7]; at = e - 2 * a3a - 7 * A;
    }
    if (dst != nullptr) dst[at] = sm[0][c];
  }
}

static int fg_check(const char* what, int64_t batch, int32_t n_fields, int32_t dim, int32_t dtype) {
  if (batch < 0) return fail(RBX_ERR_INVALID, "%s: batch=%lld", what, static_cast<long long>(batch));
  if (!rbx_fignn_step_supported(n_fields, dim))
    return fail(RBX_ERR_UNSUPPORTED, "%s: n_fields=%d in [%d,%d], dim=%d a multiple of 4 in [%d,%d], and two [n_fields][16][dim + 4] "
                "buffers plus scratch within %zu bytes of LDS", what, n_fields, kFgMinF, kFgMaxF, dim, kFgMinA, kFgMaxA, kFgLdsCap);
  if (dtype != RBX_F32) return fail(RBX_ERR_UNSUPPORTED, "%s: tensor dtype code %d (float32 only)", what, dtype);
  return RBX_OK;
}

template <typename K>
static int fg_launch(const char* what, K kernel, unsigned grid, int nw, size_t lds, hipStream_t s, const FgArgs& args) {
  const int rc = allow_lds(what, kernel, lds);
  if (rc != RBX_OK) return rc;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(64 * nw), lds, s, args);
  return RBX_OK;
}

}  // namespace rbx

extern "C" int rbx_fignn_step_supported(int32_t n_fields, int32_t dim) {
  using namespace rbx;
  return n_fields >= kFgMinF && n_fields <= kFgMaxF && dim >= kFgMinA && dim <= kFgMaxA && (dim & 3) == 0 &&
         fg_lds(n_fields, dim, true, 1, fg_tile(n_fields, dim)) <= kFgLdsCap;
}

extern "C" int rbx_fignn_step_fwd(const float* d_h, const float* d_h0, const float* d_w_attn, const float* d_w_out, const float* d_w_in,
                                  const float* d_bias_p, const float* d_w_ih, const float* d_w_hh, const float* d_b_ih,
                                  const float* d_b_hh, int64_t batch, int32_t n_fields, int32_t dim, int32_t dtype, float* d_y,
                                  float* d_graph, void* stream) {
  using namespace rbx;
  const int rc = fg_check("fignn_step_fwd", batch, n_fields, dim, dtype);
  if (rc != RBX_OK) return rc;
  if (batch == 0) return RBX_OK;
  if (!d_h || !d_h0 || !d_w_attn || !d_w_out || !d_w_in || !d_bias_p || !d_w_ih || !d_w_hh || !d_b_ih || !d_b_hh || !d_y)
    return fail(RBX_ERR_INVALID, "fignn_step_fwd: NULL tensor");
  if (!aligned16(d_h) || !aligned16(d_h0) || !aligned16(d_w_attn))
    return fail(RBX_ERR_UNSUPPORTED, "fignn_step_fwd: h, h0 and w_attn must be 16-byte aligned");
  FgArgs args = {};
  args.h = d_h; args.h0 = d_h0; args.wattn = d_w_attn; args.wout = d_w_out; args.win = d_w_in; args.biasp = d_bias_p;
  args.wih = d_w_ih; args.whh = d_w_hh; args.bih = d_b_ih; args.bhh = d_b_hh;
  args.y = d_y; args.graph = d_graph;
  args.B = batch; args.F = n_fields; args.A = dim; args.T = fg_tile(n_fields, dim); args.tshift = args.T == 16 ? 4 : 3;
  const int nw = fg_waves(n_fields, dim, false);
  const size_t lds = fg_lds(n_fields, dim, false, nw, args.T);
  hipStream_t s = as_stream(stream);
  const int lrc = dim <= 16 ? fg_launch("fignn_step_fwd", fignn_step_fwd_kernel<1>, fg_grid(batch, args.T), nw, lds, s, args)
                            : fg_launch("fignn_step_fwd", fignn_step_fwd_kernel<2>, fg_grid(batch, args.T), nw, lds, s, args);
  if (lrc != RBX_OK) return lrc;
  return check_launch("fignn_step_fwd");
}

extern "C" size_t rbx_fignn_step_bwd_workspace_size(int64_t batch, int32_t n_fields, int32_t dim) {
  using namespace rbx;
  if (batch <= 0 || !rbx_fignn_step_supported(n_fields, dim)) return 0;
  const size_t grid = fg_grid(batch, fg_tile(n_fields, dim)), nw = fg_waves(n_fields, dim, true);
  return (grid * fg_row1(n_fields, dim) + grid * nw * fg_row2(dim)) * sizeof(float);
}

extern "C" int rbx_fignn_step_bwd(const float* d_dy, const float* d_h, const float* d_h0, const float* d_w_attn, const float* d_w_out,
                                  const float* d_w_in, const float* d_bias_p, const float* d_w_ih, const float* d_w_hh,
                                  const float* d_b_ih, const float* d_b_hh, int64_t batch, int32_t n_fields, int32_t dim,
                                  int32_t dtype, float* d_dh, float* d_dh0, float* d_dw_attn, float* d_dw_out, float* d_dw_in,
                                  float* d_dbias_p, float* d_dw_ih, float* d_dw_hh, float* d_db_ih, float* d_db_hh,
                                  void* d_workspace, size_t workspace_bytes, void* stream) {
  using namespace rbx;
  const int rc = fg_check("fignn_step_bwd", batch, n_fields, dim, dtype);
  if (rc != RBX_OK) return rc;
  if (batch == 0) return RBX_OK;
  if (!d_dy || !d_h || !d_h0 || !d_w_attn || !d_w_out || !d_w_in || !d_bias_p || !d_w_ih || !d_w_hh || !d_b_ih || !d_b_hh)
    return fail(RBX_ERR_INVALID, "fignn_step_bwd: NULL tensor");
  if (!aligned16(d_h) || !aligned16(d_h0) || !aligned16(d_w_attn))
    return fail(RBX_ERR_UNSUPPORTED, "fignn_step_bwd: h, h0 and w_attn must be 16-byte aligned");
  const bool want_w = d_dw_attn || d_dw_out || d_dw_in || d_dbias_p || d_dw_ih || d_dw_hh || d_db_ih || d_db_hh;
  if (want_w && (d_workspace == nullptr || workspace_bytes < rbx_fignn_step_bwd_workspace_size(batch, n_fields, dim)))
    return fail(RBX_ERR_WORKSPACE, "fignn_step_bwd: workspace too small");
  const int nw = fg_waves(n_fields, dim, true);
  const unsigned grid = fg_grid(batch, fg_tile(n_fields, dim));
  FgArgs args = {};
  args.h = d_h; args.h0 = d_h0; args.wattn = d_w_attn; args.wout = d_w_out; args.win = d_w_in; args.biasp = d_bias_p;
  args.wih = d_w_ih; args.whh = d_w_hh; args.bih = d_b_ih; args.bhh = d_b_hh;
  args.dy = d_dy; args.dh = d_dh; args.dh0 = d_dh0;
  args.part1 = want_w ? static_cast<float*>(d_workspace) : nullptr;
  args.part2 = want_w ? args.part1 + static_cast<size_t>(grid) * fg_row1(n_fields, dim) : nullptr;
  args.B = batch; args.F = n_fields; args.A = dim; args.T = fg_tile(n_fields, dim); args.tshift = args.T == 16 ? 4 : 3;
  const size_t lds = fg_lds(n_fields, dim, true, nw, args.T);
  hipStream_t s = as_stream(stream);
  const int lrc = dim <= 16 ? fg_launch("fignn_step_bwd", fignn_step_bwd_kernel<1>, grid, nw, lds, s, args)
                            : fg_launch("fignn_step_bwd", fignn_step_bwd_kernel<2>, grid, nw, lds, s, args);
  if (lrc != RBX_OK) return lrc;
  if (want_w) {
    FgTail t = {};
    t.part1 = args.part1; t.part2 = args.part2;
    t.rows1 = static_cast<int>(grid); t.rows2 = static_cast<int>(grid) * nw;
    t.len1 = fg_row1(n_fields, dim); t.len2 = fg_row2(dim);
    t.blocks1 = (t.len1 + 15) / 16;
    t.F = n_fields; t.A = dim;
    t.dst[0] = d_dw_out; t.dst[1] = d_dw_in; t.dst[2] = d_dw_ih; t.dst[3] = d_dw_hh; t.dst[4] = d_db_ih; t.dst[5] = d_db_hh;
    t.dst[6] = d_dbias_p; t.dst[7] = d_dw_attn;
    hipLaunchKernelGGL(fignn_tail_kernel, dim3(t.blocks1 + (t.len2 + 15) / 16), dim3(256), 0, s, t);
  }
  return check_launch("fignn_step_bwd");
}
