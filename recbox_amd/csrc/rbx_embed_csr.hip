// rbx_embed_csr.hip -- K1-K3 for ragged bags: the multi-hot gather-pool over `indices` / `offsets` (CSR) and its
// deterministic backward (gfx950).
//
// Reference behaviour kept (paths relative to the reference's recbox/ package): the pooling variants of
// core/pytorch/layers/sequence.py:4-20 and third_party/rechub/basic/layers.py:176-230 over the embedding of a history,
// each exactly as rbx_pool_t defines it for padded ids (rbx_embed_fwd.hip, embed_seq_kernel) -- a bag is the history
// without its padded tail, the layout of torch.nn.EmbeddingBag.
//
// The bag walk.  Everything that reads table rows bag by bag is ONE kernel body, bag_walk_kernel<Op, G, R, NV, VEC, MODE>:
// embed_seq_kernel's mapping with the id range taken from two offset loads per lane group instead of (b * stride,
// seq_len) -- a lane group per bag, a wave task = (bag descriptor, block of 64 / SG bags) with the descriptor in SGPRs, a
// coalesced sweep of the bag's ids in chunks of 4 * SG, classify + compact into the group's LDS list, U = 4 rows in
// flight, R sub-groups for narrow rows.  The wave-uniform loop bound is the longest bag of the wave.  Chunk size, U and
// the sub-group rule are the padded kernel's own constants (rbx_rowfrag.h), so a bag is walked in the order the padded
// call walks the same live ids.  What happens to a row is the Op's business, and the four ops differ in nothing else:
//   PoolOp          (forward)          acc += row, the mean pools count; butterfly, 1 / (count + eps), store.  Bit-equal
//                                      to the padded call.  No second LDS list: 4 KB per workgroup.
//   WeightedPoolOp  (weighted forward) a weight travels with the id (a second list, 8 KB); acc += w * row; butterfly,
//                                      store.  x * 1.0f is x: all-ones weights give PoolOp's bits.
//   WeightGradOp    (weight gradient)  the position travels with the id; dw[position] = <dY[bag, slot], row>; no close.
//   MaxPoolOp       (max forward)      the position travels with the id; a row is taken elementwise where it is greater;
//                                      butterfly over (value, position) pairs, store the row and argpos.  Exact, so its
//                                      long form is bit-equal to the walk.
// Sweep, compaction and batch order exist once, so the two bit-equalities hold by construction, not by keeping copies in
// step.  check_launch still reports the ops under the names they had as separate kernels (Op::kName).
// Backward.  The positions of a descriptor's index array are its lookups.  csr_bag_map_kernel (a lane group per bag,
// coalesced stores) leaves an int32 lookup -> bag map; csr_keys_kernel builds, per sort tile, (global row, bag) pairs
// for the in-range, unmasked, non-padding ids inside a bag -- every other position gets the sentinel key the sort puts
// last and the reduce drops -- and the tile's digit counts; the radix passes, segment_reduce_kernel and the fix-ups are
// rbx_embed_bwd.hip's, with GenericPolicy over seq_len = 1 fields: the pair's value names the BAG, so the upstream
// gradient row and the mean scale (row_scale[slot * B + bag]) are read per bag and never expanded per lookup.
// User-supplied offsets are clamped to 0 <= begin <= end <= nnz before any index is read (status bit 1 when that
// changed anything): no input makes a kernel read outside indices[0, nnz).
// Per-sample weights (sum pools only; torch's per_sample_weights).  A parallel array of fp32 [nnz] weight pointers, one
// per descriptor, NULL = unweighted.  Forward: WeightedPoolOp for the descriptors that have weights, PoolOp for the rest.
// Table gradient: the weighted sort's pair value names the lookup's POSITION inside its descriptor's index array
// (csr_keys_kernel<RB, true>), and WeightedBagPolicy reads bag = map[position] and w[position] -- rbx_embed_bwd_indexed's
// indirection plus one factor; passes, reduce and fix-ups unchanged.  Weight gradient: WeightGradOp; no sort involved.
// Max pool (RBX_POOL_MAX; torch's mode="max").  Forward: MaxPoolOp, which also leaves argpos, the winner's position per output
// element (-1: the bag had no usable id, the row is zeros).  Table gradient: the position-valued sort again, and MaxBagPolicy
// reads bag = map[position] and keeps dY[bag, c] where argpos[bag, c] names that position -- WeightedBagPolicy with a mask
// instead of a factor.  argpos is only ever compared, never used as an address.
// Host side.  classify_bags sorts a call's descriptors into (float4 | scalar) x (unweighted | weighted) launches and
// refuses a dim no lane group holds before anything is written; csr_forward serves the four sum / mean forward entry
// points, csr_weight_grad the two weight-gradient ones and csr_forward_max the max forward: each keeps its own checks and
// hands its launches to walk_phases (lane groups, segments, finish).  position_reduce is the shared body of _bwd_weighted
// and _bwd_max.
#include "rbx_bwd_common.h"
#include "rbx_rowfrag.h"
#include "rbx_segreduce.h"

namespace rbx {

constexpr int kStatusBadId = 1;        // an id outside [0, vocab): as rbx_embed_fwd
constexpr int kStatusBadOffsets = 2;   // a bag's range had to be clamped

struct BagK {               // 64 B; RBX_MAX_BAGS of them (2 KiB) travel in the kernarg segment
  const void* indices;
  const void* offsets;
  const float* table;
  long long idx_stride;
  int nnz;
  int vocab;
  int mask_id;              // kNoId when unset
  int pad_id;
  int out_off;
  short dim;
  unsigned char idx_dtype, off_dtype, pool, slot;
  short reserved;
  float eps;
};
static_assert(sizeof(BagK) == 64, "BagK must stay 64 bytes");
struct BagPack { BagK f[RBX_MAX_BAGS]; };
struct BagLookups { unsigned lk_off[RBX_MAX_BAGS]; };   // first lookup of every bag descriptor in the call's sort
template <class T>
struct BagPtrs { T* p[RBX_MAX_BAGS]; };                 // one fp32 [nnz] array per descriptor of a BagPack, same order
using BagWeights = BagPtrs<const float>;                // per-sample weights
using BagWeightGrads = BagPtrs<float>;                  // ... and where their gradients go

// [begin, end) of bag b, clamped into [0, nnz]; *bad: the clamp changed something
__device__ __forceinline__ void bag_range(const BagK& fd, long long b, int* begin, int* end, bool* bad) {
  long long o0, o1;
  if (fd.off_dtype == RBX_I64) {
    o0 = static_cast<const long long*>(fd.offsets)[b];
    o1 = static_cast<const long long*>(fd.offsets)[b + 1];
  } else {
    o0 = static_cast<const int*>(fd.offsets)[b];
    o1 = static_cast<const int*>(fd.offsets)[b + 1];
  }
  const long long n = fd.nnz;
  const long long lo = o0 < 0 ? 0 : (o0 > n ? n : o0);
  const long long hi = o1 < lo ? lo : (o1 > n ? n : o1);
  *begin = static_cast<int>(lo);
  *end = static_cast<int>(hi);
  *bad = (lo != o0) || (hi != o1);
}

// ---- the long-bag form: a bag of >= T ids is cut into segments of RBX_CSR_SEGMENT ids, a wave per segment ---------------
// MODE of bag_walk_kernel: kWalk = a lane group per bag whatever its length (the entry points without `_long`);
// kHandOff = the same, but a group whose bag has L >= T appends a record to the workspace and neither sweeps nor stores;
// kSegments = a wave task is one segment of a recorded bag: the wave's lane groups take consecutive S / (64 / G) ids each
// and walk them exactly as a lane group walks a bag (chunk / list / U / R), the closing butterfly runs over the whole wave,
// and the partial row (and count) goes to the workspace.  csr_long_finish_kernel sums a bag's partials in ascending
// segment order: a fixed order, so two runs give the same bits.
// One 64-bit atomicAdd per long bag hands out (record index, first segment slot) together: records are ordered by their
// first slot and a segment task finds its bag by binary search.  Capacities are static (long_plan); well-formed offsets
// cannot exceed them, and a bag whose indices come back beyond either is walked by its lane group in that same launch.
constexpr int kWalk = 0, kHandOff = 1, kSegments = 2;
constexpr int kSeg = RBX_CSR_SEGMENT;

struct LongRec { int desc, cls, bag, begin, end, seg0, r0, r1; };   // 32 B; begin == end: refused (walked by its lane group)
struct LongArgs {
  unsigned long long* hdr;  // high word: long bags, low word: segments handed out
  LongRec* recs;            // [cap_bags]
  float* part;              // [cap_segs][pstride] partial rows
  float* pcnt;              // [cap_segs] partial counts of the mean pools
  int T, cap_bags, cap_segs, pstride;
  int cls;                  // the launch's class (float4 | scalar, unweighted | weighted): a segment kernel takes its own
};

// one lane of the group; returns 1 when the bag now belongs to the segment kernel
__device__ __forceinline__ int long_append(const LongArgs& la, int desc, long long bag, int begin, int end) {
  const unsigned nseg = static_cast<unsigned>((end - begin + kSeg - 1) / kSeg);
  const unsigned long long cur = __hip_atomic_load(la.hdr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if ((cur >> 32) >= static_cast<unsigned long long>(la.cap_bags) ||
      (cur & 0xFFFFFFFFull) + nseg > static_cast<unsigned long long>(la.cap_segs))
    return 0;                                             // already full (overlapping bags): the counters stop growing
  const unsigned long long old = atomicAdd(la.hdr, (1ull << 32) | nseg);
  const unsigned long long bi = old >> 32, s0 = old & 0xFFFFFFFFull;
  if (bi >= static_cast<unsigned long long>(la.cap_bags)) return 0;
  const bool ok = s0 + nseg <= static_cast<unsigned long long>(la.cap_segs);
  LongRec r;
  r.desc = desc;
  r.cls = la.cls;
  r.bag = static_cast<int>(bag);
  r.begin = ok ? begin : 0;
  r.end = ok ? end : 0;
  r.seg0 = static_cast<int>(s0 < 0x7FFFFFFFull ? s0 : 0x7FFFFFFFull);
  r.r0 = r.r1 = 0;
  la.recs[bi] = r;
  return ok ? 1 : 0;
}

// the counts a later kernel of the call reads, clamped to the capacities
__device__ __forceinline__ void long_counts(const LongArgs& la, int* n_bags, long long* n_segs) {
  const unsigned long long h = *la.hdr;
  const unsigned long long nb = h >> 32, ns = h & 0xFFFFFFFFull;
  *n_bags = static_cast<int>(nb < static_cast<unsigned long long>(la.cap_bags) ? nb : la.cap_bags);
  *n_segs = (*n_bags == 0) ? 0 : static_cast<long long>(ns < static_cast<unsigned long long>(la.cap_segs) ? ns : la.cap_segs);
}

// the record of segment slot s (wave-uniform: the fields come back in SGPRs): the last one with seg0 <= s
__device__ __forceinline__ LongRec long_find(const LongArgs& la, int n_bags, long long s) {
  int lo = 0, hi = n_bags - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (la.recs[mid].seg0 <= s) lo = mid; else hi = mid - 1;
  }
  const LongRec v = la.recs[lo];
  LongRec r;
  r.desc = __builtin_amdgcn_readfirstlane(v.desc);
  r.cls = __builtin_amdgcn_readfirstlane(v.cls);
  r.bag = __builtin_amdgcn_readfirstlane(v.bag);
  r.begin = __builtin_amdgcn_readfirstlane(v.begin);
  r.end = __builtin_amdgcn_readfirstlane(v.end);
  r.seg0 = __builtin_amdgcn_readfirstlane(v.seg0);
  r.r0 = r.r1 = 0;
  return r;
}

// [begin, end) of lane group `gi` (of GPW per wave) inside segment slot s of record r; empty when the slot is not r's
template <int GPW>
__device__ __forceinline__ void long_sub_range(const LongRec& r, long long s, int gi, int* begin, int* end) {
  constexpr int kSub = kSeg / GPW;                        // a multiple of the group's chunk 4 * G (G = 64 / GPW >= 16)
  const long long seg_b = static_cast<long long>(r.begin) + (s - r.seg0) * kSeg;
  const long long seg_e = seg_b + kSeg < r.end ? seg_b + kSeg : r.end;
  long long gb = seg_b + static_cast<long long>(gi) * kSub;
  if (s < r.seg0 || gb > seg_e) gb = seg_e;
  if (gb < r.begin) gb = r.begin;                         // (an empty record: begin == end)
  long long ge = gb + kSub < seg_e ? gb + kSub : seg_e;
  if (ge < gb) ge = gb;
  *begin = static_cast<int>(gb);
  *end = static_cast<int>(ge);
}

// ---- the bag walk: one kernel body, an op per use ----------------------------------------------------------------------
// bag_walk_kernel is embed_seq_kernel's mapping over [begin, end) of a bag; kSeqWaves, kSeqU, kSeqIpl and seq_group_lanes
// (rbx_rowfrag.h) are that kernel's own, so chunks, batches and sub-group counts are equal by construction.  An op says
// what happens to a row once it is in registers:
//   Args      what the op reads and writes, passed to the kernel by value;
//   Payload   the value that travels with an id through the LDS list (kHasPayload = false: no second list at all);
//   Bag       the state of one (lane group, bag): open() per bag, payload() in the id sweep, row() per loaded row,
//             close() after the last chunk.  `owner` lanes store: the first sub-group of a live bag that was not handed
//             over; in kSegments the first W lanes of the wave, and the row goes to partial slot t of the workspace.
// Every lane of the wave reaches open(), row() and close() together (the loop bounds are wave-uniform), so they may shuffle.
struct NoPayload {};

// sum / mean pools: acc += row, the mean pools count as rbx_pool_t says; close = butterfly, 1 / (count + eps), store
struct PoolOp {
  static constexpr const char* kName = "embed_csr_kernel";
  static constexpr bool kMasksIds = false;   // mask_id counts for the _ID pools only (true: whenever it is set)
  static constexpr bool kHasPayload = false;
  using Payload = NoPayload;
  struct Args {
    float* out;
    long long stride_b;
    float* row_scale;       // NULL: not wanted
  };
  template <int W, int NV, bool VEC>
  struct Bag {
    using Frag = RowFrag<W, NV, VEC>;
    Frag acc;
    float count;
    __device__ __forceinline__ void open(const Args&, const BagK&, int, long long, bool, int) {
      acc.zero();
      count = 0.f;
    }
    __device__ __forceinline__ void row(const BagK& fd, Frag& r, int id, Payload, int) {
      acc.add(r);
      if (fd.pool == RBX_POOL_MEAN_VALUE) {
        const float sm = group_sum<W>(r.hsum());          // value mask: row sum != 0
        count += (sm != 0.f) ? 1.f : 0.f;
      } else if (fd.pool == RBX_POOL_MEAN_ID) {
        count += (id >= 0) ? 1.f : 0.f;
      }
    }
    template <int MODE, int G>
    __device__ __forceinline__ void close(const Args& a, const LongArgs& la, const BagK& fd, long long t, long long b, long long B,
                                          bool owner, int lane_w) {
#pragma unroll
      for (int o = W; o < (MODE == kSegments ? 64 : G); o <<= 1) {   // every lane joins the butterfly (segments: the whole wave)
        acc.xor_add(o);
        count += __shfl_xor(count, o, 64);
      }
      if (!owner) return;
      if constexpr (MODE == kSegments) {                  // t < cap_segs (long_counts); the finish applies the mean scale
        acc.store(la.part + t * la.pstride, fd.dim, lane_w);
        if (lane_w == 0) la.pcnt[t] = count;
      } else {
        if (fd.pool == RBX_POOL_MEAN_VALUE || fd.pool == RBX_POOL_MEAN_ID) {
          const float inv = 1.0f / (count + fd.eps);      // an empty bag: 0 * (1 / eps) = 0
          acc.scale(inv);
          if (a.row_scale != nullptr && lane_w == 0) a.row_scale[static_cast<long long>(fd.slot) * B + b] = inv;
        }
        acc.store(a.out + b * a.stride_b + fd.out_off, fd.dim, lane_w);
      }
    }
  };
};

// sum pools with one factor per lookup: the weight is loaded beside the id, compacted beside it and multiplied into the
// row before the add.  x * 1.0f is x: all-ones weights give PoolOp's bits.
struct WeightedPoolOp {
  static constexpr const char* kName = "embed_csr_weighted_kernel";
  static constexpr bool kMasksIds = false;
  static constexpr bool kHasPayload = true;
  using Payload = float;
  struct Args {
    BagWeights w;
    float* out;
    long long stride_b;
  };
  template <int W, int NV, bool VEC>
  struct Bag {
    using Frag = RowFrag<W, NV, VEC>;
    Frag acc;
    const float* __restrict__ wsrc;
    __device__ __forceinline__ void open(const Args& a, const BagK&, int f, long long, bool, int) {
      acc.zero();
      wsrc = a.w.p[f];
    }
    __device__ __forceinline__ float payload(long long pos, bool live) const { return live ? wsrc[pos] : 0.f; }
    __device__ __forceinline__ void row(const BagK&, Frag& r, int, float w, int) {
      r.scale(w);
      acc.add(r);
    }
    template <int MODE, int G>
    __device__ __forceinline__ void close(const Args& a, const LongArgs& la, const BagK& fd, long long t, long long b, long long,
                                          bool owner, int lane_w) {
#pragma unroll
      for (int o = W; o < (MODE == kSegments ? 64 : G); o <<= 1) acc.xor_add(o);   // every lane joins the butterfly
      if (!owner) return;
      if constexpr (MODE == kSegments) acc.store(la.part + t * la.pstride, fd.dim, lane_w);
      else acc.store(a.out + b * a.stride_b + fd.out_off, fd.dim, lane_w);
    }
  };
};

// weight gradient: dw[j] = <dY[bag, slot], table[id_j]>.  The bag's dY fragment is loaded once, the ids travel with their
// positions, the dot is reduced over the W lanes that hold a row and stored by the first of them; nothing to combine at the
// end, so a handed-over bag is an empty one here.  Only usable positions are written: the host clears dw[0, nnz) in front
// of the launch, so masked and out-of-range ids and the positions outside every bag read 0.
template <int W, int NV>
__device__ __forceinline__ float row_dot(const RowFrag<W, NV, true>& a, const RowFrag<W, NV, true>& b) {
  float s = 0.f;
#pragma unroll
  for (int u = 0; u < NV; ++u)
    s += (a.a[u].v.x * b.a[u].v.x + a.a[u].v.y * b.a[u].v.y) + (a.a[u].v.z * b.a[u].v.z + a.a[u].v.w * b.a[u].v.w);
  return s;
}
template <int W, int NV>
__device__ __forceinline__ float row_dot(const RowFrag<W, NV, false>& a, const RowFrag<W, NV, false>& b) {
  float s = 0.f;
#pragma unroll
  for (int u = 0; u < NV; ++u) s += a.a[u].v * b.a[u].v;
  return s;
}

struct WeightGradOp {
  static constexpr const char* kName = "csr_weight_grad_kernel";
  static constexpr bool kMasksIds = false;
  static constexpr bool kHasPayload = true;
  using Payload = int;
  struct Args {
    BagWeightGrads dw;
    const float* dout;
    long long stride_b;
  };
  template <int W, int NV, bool VEC>
  struct Bag {
    using Frag = RowFrag<W, NV, VEC>;
    Frag dy;
    float* __restrict__ dw;
    __device__ __forceinline__ void open(const Args& a, const BagK& fd, int f, long long b, bool alive, int lane_w) {
      dw = a.dw.p[f];
      dy.zero();
      if (alive) dy.load(a.dout + b * a.stride_b + fd.out_off, fd.dim, lane_w);
    }
    __device__ __forceinline__ int payload(long long pos, bool) const { return static_cast<int>(pos); }   // < end <= nnz
    __device__ __forceinline__ void row(const BagK&, Frag& r, int id, int pos, int lane_w) {
      const float d = group_sum<W>(row_dot(r, dy));
      if (id >= 0 && lane_w == 0) dw[pos] = d;
    }
    template <int MODE, int G>
    __device__ __forceinline__ void close(const Args&, const LongArgs&, const BagK&, long long, long long, long long, bool, int) {}
  };
};


// max pool: a row is taken elementwise where nothing has been taken yet or where it is strictly greater, and the position of
// the id it came with is kept per element.  A lane group meets its own ids in ascending position, so within a sub-group
// strict > alone is "first occurrence wins".  close() combines (value, position) pairs across the R sub-groups -- in
// kSegments across the whole wave -- by an xor butterfly under one lexicographic rule: the greater value wins, on equal
// values the lower position, and "nothing taken" (position -1) loses to anything.  That rule is a total order on the pairs
// of a bag (positions are distinct), so its maximum does not depend on the order of the combination: the result is "the
// lowest position among the maxima" by construction, whatever R, the mode or the threshold.  Table values are finite
// (NaN / +-inf are outside the contract).  mask_id is honoured whenever it is set: kNoId equals no in-range id.
struct MaxPoolOp {
  static constexpr const char* kName = "embed_csr_max_kernel";
  static constexpr bool kMasksIds = true;
  static constexpr bool kHasPayload = true;
  using Payload = int;
  struct Args {
    float* out;
    long long stride_b;
    int* argpos;            // [batch, arg_stride]: the winner's position per output element, -1 where there is none
    long long arg_stride;
    int* parg;              // kSegments: [cap_segs][pstride] partial argpos rows beside LongArgs::part
    int arg_vec;            // argpos rows take 16-byte stores
  };
  template <int W, int NV, bool VEC>
  struct Bag {
    using Frag = RowFrag<W, NV, VEC>;
    static constexpr int E = Frag::kElems;
    Frag val;
    int pos[E];
    bool any;
    __device__ __forceinline__ void open(const Args&, const BagK&, int, long long, bool, int) {
      val.zero();
#pragma unroll
      for (int q = 0; q < E; ++q) pos[q] = -1;
      any = false;
    }
    __device__ __forceinline__ int payload(long long p, bool) const { return static_cast<int>(p); }   // < end <= nnz
    __device__ __forceinline__ void row(const BagK&, Frag& r, int id, int p, int) {
      if (id < 0) return;                                   // (an empty slot of the batch)
#pragma unroll
      for (int q = 0; q < E; ++q) {
        const bool take = !any || r.at(q) > val.at(q);
        val.at(q) = take ? r.at(q) : val.at(q);
        pos[q] = take ? p : pos[q];
      }
      any = true;
    }
    static __device__ __forceinline__ void store_pos(const int (&pos)[E], int* row, int dim, int lane_w, bool vec) {
      constexpr int WD = Frag::W;
#pragma unroll
      for (int u = 0; u < NV; ++u) {
        const int e = (lane_w + u * W) * WD;
        if (e >= dim) continue;
        if constexpr (VEC) {
          if (vec) {
            *reinterpret_cast<int4*>(row + e) = make_int4(pos[u * 4], pos[u * 4 + 1], pos[u * 4 + 2], pos[u * 4 + 3]);
          } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) row[e + k] = pos[u * 4 + k];
          }
        } else {
          row[e] = pos[u];
        }
      }
    }
    template <int MODE, int G>
    __device__ __forceinline__ void close(const Args& a, const LongArgs& la, const BagK& fd, long long t, long long b, long long,
                                          bool owner, int lane_w) {
#pragma unroll
      for (int o = W; o < (MODE == kSegments ? 64 : G); o <<= 1) {   // every lane joins the butterfly (segments: the whole wave)
        Frag ov = val.xor_get(o);
#pragma unroll
        for (int q = 0; q < E; ++q) {
          const int op = __shfl_xor(pos[q], o, 64);
          const float x = ov.at(q), v = val.at(q);
          const bool take = op >= 0 && (pos[q] < 0 || x > v || (x == v && op < pos[q]));
          val.at(q) = take ? x : v;
          pos[q] = take ? op : pos[q];
        }
      }
      if (!owner) return;
      // an element nothing was taken for still holds the 0 of open(): the zero row of a bag without a usable id
      if constexpr (MODE == kSegments) {                  // t < cap_segs (long_counts); pstride is a multiple of 4
        val.store(la.part + t * la.pstride, fd.dim, lane_w);
        store_pos(pos, a.parg + t * la.pstride, fd.dim, lane_w, true);
      } else {
        val.store(a.out + b * a.stride_b + fd.out_off, fd.dim, lane_w);
        store_pos(pos, a.argpos + b * a.arg_stride + fd.out_off, fd.dim, lane_w, a.arg_vec != 0);
      }
    }
  };
};

// A lane group per bag, a wave task = (bag descriptor, block of 64 / G bags) with the descriptor in SGPRs; in kSegments a
// wave task is one segment slot.  Per chunk of 4 * G ids: (1a) one coalesced sweep of the ids (and the op's payload),
// (1b) classify + compact into the group's LDS list, (2) the list walked U rows at a time, R sub-groups side by side.
template <class Op, int G, int R, int NV, bool VEC, int MODE>
__global__ __launch_bounds__(256, kSeqWaves) void bag_walk_kernel(const BagPack P, const typename Op::Args A, const int F,
                                                                  const long long B, int* __restrict__ status,
                                                                  const LongArgs LA) {
  constexpr int W = G / R;                                // lanes that hold one row
  using Frag = RowFrag<W, NV, VEC>;
  using Pay = typename Op::Payload;
  constexpr int U = kSeqU;
  constexpr int IPL = kSeqIpl;
  constexpr int C = G * IPL;                              // lookups per chunk
  constexpr int GPB = 256 / G;
  __shared__ int s_id[GPB][C];
  const int lane_w = threadIdx.x % W;
  const int sub = (threadIdx.x % G) / W;
  const int lane_g = threadIdx.x % G;
  const int gidx = threadIdx.x / G;
  const int gshift = (threadIdx.x & 63) & ~(G - 1);       // first lane of the group inside its wave
  const unsigned long long gmask = (G == 64) ? ~0ull : ((1ull << G) - 1ull);
  const unsigned long long below = (1ull << lane_g) - 1ull;
  volatile int* my_id = s_id[gidx];
  volatile Pay* my_pay = nullptr;
  if constexpr (Op::kHasPayload) {                        // the second list exists only for an op that has something to put there
    __shared__ Pay s_pay[GPB][C];
    my_pay = s_pay[gidx];
  }
  constexpr int GPW = 64 / G;
  const long long tasks_per_bag = (B + GPW - 1) / GPW;
  long long ntasks = tasks_per_bag * F;
  int n_long = 0;
  if constexpr (MODE == kSegments) long_counts(LA, &n_long, &ntasks);    // a wave task = one segment slot
  const long long nwaves = static_cast<long long>(gridDim.x) * 4;
  for (long long t = static_cast<long long>(blockIdx.x) * 4 + threadIdx.x / 64; t < ntasks; t += nwaves) {
    int f, begin = 0, end = 0;
    long long b;
    bool alive;
    if constexpr (MODE == kSegments) {
      const LongRec rec = long_find(LA, n_long, t);
      if (rec.cls != LA.cls || static_cast<unsigned>(rec.desc) >= static_cast<unsigned>(F)) continue;
      f = rec.desc;
      b = rec.bag;
      alive = true;
      long_sub_range<GPW>(rec, t, (threadIdx.x & 63) / G, &begin, &end);
    } else {
      f = __builtin_amdgcn_readfirstlane(static_cast<int>(t / tasks_per_bag));
      b = (t - f * tasks_per_bag) * GPW + (threadIdx.x & 63) / G;
      alive = b < B;
    }
    const BagK& fd = P.f[f];
    const int pool = fd.pool, dim = fd.dim, dt = fd.idx_dtype;
    const bool id_pool = Op::kMasksIds || (pool == RBX_POOL_MEAN_ID || pool == RBX_POOL_SUM_ID);
    if (MODE != kSegments && alive) {
      bool bad;
      bag_range(fd, b, &begin, &end, &bad);
      if (bad && lane_g == 0 && status != nullptr) atomicOr(status, kStatusBadOffsets);
    }
    typename Op::template Bag<W, NV, VEC> bag;
    bag.open(A, fd, f, b, alive, lane_w);
    int L = end - begin;
    bool handed = false;                                  // the bag went to the segment kernel: no sweep, no store here
    if constexpr (MODE == kHandOff) {
      int took = 0;
      if (alive && lane_g == 0 && L >= LA.T) took = long_append(LA, fd.slot, b, begin, end);
      handed = __shfl(took, 0, G) != 0;
      if (handed) L = 0;
    }
    int Lmax = L;                                         // wave-uniform number of chunks: the longest bag of the wave
#pragma unroll
    for (int o = 32; o >= G && o > 0; o >>= 1) {
      const int other = __shfl_xor(Lmax, o, 64);
      Lmax = other > Lmax ? other : Lmax;
    }
    for (int c0 = 0; c0 < Lmax; c0 += C) {
      long long raw[IPL];
      Pay pay[IPL];
#pragma unroll
      for (int i = 0; i < IPL; ++i) {                     // (1a) one coalesced sweep of id loads; l < L <=> inside [begin, end)
        const int l = c0 + i * G + lane_g;
        raw[i] = (l < L) ? load_raw(fd.indices, (static_cast<long long>(begin) + l) * fd.idx_stride, dt) : 0;
        if constexpr (Op::kHasPayload) pay[i] = bag.payload(static_cast<long long>(begin) + l, l < L);
      }
      int nvalid = 0;
#pragma unroll
      for (int i = 0; i < IPL; ++i) {                     // (1b) classify + compact
        const int l = c0 + i * G + lane_g;
        const long long id = decode_id(raw[i], dt);
        const bool live = l < L;
        const bool in_range = id >= 0 && id < fd.vocab;
        if (live && !in_range && status != nullptr) atomicOr(status, kStatusBadId);
        const bool use = live && in_range && !(id_pool && id == fd.mask_id);
        const unsigned long long m = (__ballot(use) >> gshift) & gmask;
        if (use) {
          const int at = nvalid + __popcll(m & below);
          my_id[at] = static_cast<int>(id);
          if constexpr (Op::kHasPayload) my_pay[at] = pay[i];
        }
        nvalid += __popcll(m);
      }
      __builtin_amdgcn_wave_barrier();
      int nmax = nvalid;                                   // wave-uniform batch count
#pragma unroll
      for (int o = 32; o >= G && o > 0; o >>= 1) {
        const int other = __shfl_xor(nmax, o, 64);
        nmax = other > nmax ? other : nmax;
      }
      for (int k0 = 0; k0 < nmax; k0 += U * R) {          // (2) dense row batches
        int idu[U];
        Pay pu[U] = {};
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int k = k0 + u * R + sub;
          idu[u] = (k < nvalid) ? my_id[k] : -1;
          if constexpr (Op::kHasPayload) pu[u] = (k < nvalid) ? my_pay[k] : Pay(0);
        }
        Frag r[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          r[u].zero();
          if (idu[u] >= 0) r[u].load(fd.table + static_cast<long long>(idu[u]) * dim, dim, lane_w);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) bag.row(fd, r[u], idu[u], pu[u], lane_w);
      }
      __builtin_amdgcn_wave_barrier();
    }
    const bool owner = (MODE == kSegments) ? (threadIdx.x & 63) < W : (alive && sub == 0 && !handed);
    bag.template close<MODE, G>(A, LA, fd, t, b, B, owner, lane_w);
  }
}

// the segment launches' grid: fixed, grid-striding over the segment count in the workspace header
constexpr int kSegBlocks = kCUs * 4;

template <class Op, int G, int NV, bool VEC, int MODE>
static int launch_bag_walk(const BagPack& pack, int F, int64_t B, const typename Op::Args& args, int* status, hipStream_t s,
                           const LongArgs& la) {
  constexpr int SG = seq_group_lanes(G);                  // lanes per bag
  long long blocks = ((B + 64 / SG - 1) / (64 / SG) * F + 3) / 4;   // 4 wave tasks per workgroup
  const long long cap = static_cast<long long>(kCUs) * 64;
  if (blocks > cap) blocks = cap;
  if (blocks < 1) blocks = 1;
  if (MODE == kSegments) blocks = kSegBlocks;
  hipLaunchKernelGGL((bag_walk_kernel<Op, SG, SG / G, NV, VEC, MODE>), dim3(static_cast<unsigned>(blocks)), dim3(256), 0, s, pack,
                     args, F, static_cast<long long>(B), status, la);
  return check_launch(Op::kName);
}

template <class Op, bool VEC, int MODE>
static int dispatch_bag_walk(int units, const BagPack& pack, int F, int64_t B, const typename Op::Args& args, int* status,
                             hipStream_t s, const LongArgs& la) {
  switch (pow2_ceil(units)) {
    case 1: return launch_bag_walk<Op, 1, 1, VEC, MODE>(pack, F, B, args, status, s, la);
    case 2: return launch_bag_walk<Op, 2, 1, VEC, MODE>(pack, F, B, args, status, s, la);
    case 4: return launch_bag_walk<Op, 4, 1, VEC, MODE>(pack, F, B, args, status, s, la);
    case 8: return launch_bag_walk<Op, 8, 1, VEC, MODE>(pack, F, B, args, status, s, la);
    case 16: return launch_bag_walk<Op, 16, 1, VEC, MODE>(pack, F, B, args, status, s, la);
    case 32: return launch_bag_walk<Op, 32, 1, VEC, MODE>(pack, F, B, args, status, s, la);
    case 64: return launch_bag_walk<Op, 64, 1, VEC, MODE>(pack, F, B, args, status, s, la);
    case 128: return launch_bag_walk<Op, 64, 2, VEC, MODE>(pack, F, B, args, status, s, la);
    case 256: return launch_bag_walk<Op, 64, 4, VEC, MODE>(pack, F, B, args, status, s, la);
    default: return fail(RBX_ERR_UNSUPPORTED, "embedding dim too large for one lane group (units=%d)", units);
  }
}

// the (float4 | scalar) x mode choice of a launch, made at run time
template <class Op>
static int bag_walk(bool vec, int mode, int units, const BagPack& pack, int F, int64_t B, const typename Op::Args& args,
                    int* status, hipStream_t s, const LongArgs& la) {
  switch (mode) {
    case kWalk: return vec ? dispatch_bag_walk<Op, true, kWalk>(units, pack, F, B, args, status, s, la)
                           : dispatch_bag_walk<Op, false, kWalk>(units, pack, F, B, args, status, s, la);
    case kHandOff: return vec ? dispatch_bag_walk<Op, true, kHandOff>(units, pack, F, B, args, status, s, la)
                              : dispatch_bag_walk<Op, false, kHandOff>(units, pack, F, B, args, status, s, la);
    default: return vec ? dispatch_bag_walk<Op, true, kSegments>(units, pack, F, B, args, status, s, la)
                        : dispatch_bag_walk<Op, false, kSegments>(units, pack, F, B, args, status, s, la);
  }
}

// a weight array (or a weight gradient) belongs to a sum pool: torch's rule for per_sample_weights
static int check_weighted_pools(const rbx_bag_t* bags, int n, const void* const* per_bag, const char* what) {
  for (int i = 0; per_bag != nullptr && i < n; ++i)
    if (per_bag[i] != nullptr && bags[i].pool != RBX_POOL_SUM && bags[i].pool != RBX_POOL_SUM_ID)
      return fail(RBX_ERR_UNSUPPORTED, "bag %d: %s with pool mode %d; per-sample weights go with RBX_POOL_SUM / RBX_POOL_SUM_ID "
                  "only (weighted mean pools are not implemented)", i, what, bags[i].pool);
  return RBX_OK;
}

// the sum / mean entry points and everything with weights: a max pool has calls of its own (rbx_embed_csr_fwd_max / _bwd_max)
static int check_no_max(const rbx_bag_t* bags, int n, const char* who) {
  for (int i = 0; bags != nullptr && i < n; ++i)
    if (bags[i].pool == RBX_POOL_MAX)
      return fail(RBX_ERR_UNSUPPORTED, "%s: bag %d is a max pool; it goes through rbx_embed_csr_fwd_max / rbx_embed_csr_bwd_max "
                  "(and takes no per-sample weights)", who, i);
  return RBX_OK;
}
static int check_all_max(const rbx_bag_t* bags, int n, const char* who) {
  for (int i = 0; bags != nullptr && i < n; ++i)
    if (bags[i].pool != RBX_POOL_MAX)
      return fail(RBX_ERR_UNSUPPORTED, "%s: bag %d has pool mode %d; every descriptor of the call must be RBX_POOL_MAX", who, i,
                  bags[i].pool);
  return RBX_OK;
}

static int compact(int64_t v) { return (v == RBX_NO_ID || v < INT_MIN || v > INT_MAX) ? kNoId : static_cast<int>(v); }

// The size checks of pack_bags and long_plan (which also sees descriptors whose pointers are not set yet): i < 0 the
// call's bags / n / batch, otherwise the dim / nnz of descriptor i.
static int check_sizes(const rbx_bag_t* bags, int n, int64_t batch, int i) {
  if (i < 0) {
    if (bags == nullptr) return fail(RBX_ERR_INVALID, "bags is NULL");
    if (n <= 0 || n > RBX_MAX_BAGS) return fail(RBX_ERR_INVALID, "n_bags=%d not in [1,%d]", n, RBX_MAX_BAGS);
    if (batch < 0) return fail(RBX_ERR_INVALID, "negative batch");
    if (batch > static_cast<int64_t>(kLocalMask)) return fail(RBX_ERR_UNSUPPORTED, "batch=%lld exceeds 2^26 bags per call", (long long)batch);
    return RBX_OK;
  }
  const rbx_bag_t& g = bags[i];
  if (g.dim <= 0 || g.dim > 1024) return fail(RBX_ERR_UNSUPPORTED, "bag %d: dim=%d not in [1,1024]", i, g.dim);
  if (g.nnz < 0 || g.nnz > static_cast<int64_t>(kLocalMask))
    return fail(RBX_ERR_UNSUPPORTED, "bag %d: nnz=%lld not in [0, 2^26]", i, (long long)g.nnz);
  return RBX_OK;
}

// Validate the public descriptors; convert descriptor i into out[i] (slot = i).
static int pack_bags(const rbx_bag_t* bags, int n, int64_t batch, BagK* out) {
  int rc = check_sizes(bags, n, batch, -1);
  if (rc != RBX_OK) return rc;
  unsigned long long total = 0;
  for (int i = 0; i < n; ++i) {
    const rbx_bag_t& g = bags[i];
    if (g.pool == RBX_POOL_NONE || g.pool == RBX_POOL_CONCAT)
      return fail(RBX_ERR_UNSUPPORTED, "bag %d: pool mode %d keeps one slot per id; ragged bags are pooled (sum / mean / max)", i, g.pool);
    if (g.pool < RBX_POOL_NONE || g.pool > RBX_POOL_MAX) return fail(RBX_ERR_INVALID, "bag %d: bad pool mode %d", i, g.pool);
    rc = check_sizes(bags, n, batch, i);
    if (rc != RBX_OK) return rc;
    if (g.nnz > 0 && g.indices == nullptr) return fail(RBX_ERR_INVALID, "bag %d: indices is NULL", i);
    if (g.offsets == nullptr) return fail(RBX_ERR_INVALID, "bag %d: offsets is NULL", i);
    if (g.table == nullptr) return fail(RBX_ERR_INVALID, "bag %d: table is NULL", i);
    if (g.indices_dtype < RBX_I32 || g.indices_dtype > RBX_F64) return fail(RBX_ERR_INVALID, "bag %d: bad indices_dtype", i);
    if (g.offsets_dtype != RBX_I32 && g.offsets_dtype != RBX_I64)
      return fail(RBX_ERR_INVALID, "bag %d: offsets must be int32 or int64", i);
    if (g.vocab <= 0 || g.vocab > INT_MAX) return fail(RBX_ERR_INVALID, "bag %d: vocab=%lld", i, (long long)g.vocab);
    if (g.out_off < 0 || g.out_off > INT_MAX) return fail(RBX_ERR_INVALID, "bag %d: out_off", i);
    total += static_cast<unsigned long long>(g.nnz);
    BagK& k = out[i];
    k.indices = g.indices;
    k.offsets = g.offsets;
    k.table = g.table;
    k.idx_stride = g.indices_stride;
    k.nnz = static_cast<int>(g.nnz);
    k.vocab = static_cast<int>(g.vocab);
    k.mask_id = compact(g.mask_id);
    k.pad_id = compact(g.padding_idx);
    k.out_off = static_cast<int>(g.out_off);
    k.dim = static_cast<short>(g.dim);
    k.idx_dtype = static_cast<unsigned char>(g.indices_dtype);
    k.off_dtype = static_cast<unsigned char>(g.offsets_dtype);
    k.pool = static_cast<unsigned char>(g.pool);
    k.slot = static_cast<unsigned char>(i);
    k.reserved = 0;
    k.eps = g.eps;
  }
  if (total >= (1ull << 31)) return fail(RBX_ERR_UNSUPPORTED, "nnz of the call = %llu, limit 2^31", total);
  return RBX_OK;
}

static bool bag_vec_ok(const rbx_bag_t& g, const float* out, int64_t stride_b) {
  if (g.dim % 4 != 0 || g.out_off % 4 != 0 || stride_b % 4 != 0) return false;
  if ((reinterpret_cast<uintptr_t>(g.table) & 15) != 0) return false;
  if ((reinterpret_cast<uintptr_t>(out) & 15) != 0) return false;
  return true;
}

// ---- backward: lookup -> bag map, (row, bag) pairs -----------------------------------------------------------------
// grid (x, bag descriptors of the plan); 16 lane groups of 16 lanes per workgroup, a group per bag: the bags of a
// descriptor are consecutive ranges of its index array, so neighbouring groups store neighbouring runs.
__global__ __launch_bounds__(256) void csr_bag_map_kernel(const BagPack P, const BagLookups LK, const long long B,
                                                          int* __restrict__ map, int* __restrict__ status) {
  const BagK& fd = P.f[blockIdx.y];
  int* __restrict__ my = map + LK.lk_off[blockIdx.y];
  const int lane = threadIdx.x & 15;
  for (long long b = static_cast<long long>(blockIdx.x) * 16 + (threadIdx.x >> 4); b < B;
       b += static_cast<long long>(gridDim.x) * 16) {
    int begin, end;
    bool bad;
    bag_range(fd, b, &begin, &end, &bad);
    if (bad && lane == 0 && status != nullptr) atomicOr(status, kStatusBadOffsets);
    for (int j = begin + lane; j < end; j += 16) my[j] = static_cast<int>(b);
  }
}

// build_keys_kernel's tile structure (one workgroup per sort tile, the tile's digit counts out of the same pass) over
// lookups that are positions of index arrays: position j of descriptor `lo` is a pair iff the map names a bag for it.
// POS (the weighted sort): the pair's value names the position inside the descriptor's index array instead of the bag.
template <int RB, bool POS = false>
__global__ __launch_bounds__(kSortThreads) void csr_keys_kernel(const KeyPack P, const int n_cat, const SegPack S,
                                                                const unsigned sentinel, const int* __restrict__ map,
                                                                unsigned* __restrict__ keys0, unsigned* __restrict__ vals0,
                                                                unsigned* __restrict__ keys1, unsigned* __restrict__ vals1,
                                                                int* __restrict__ status, unsigned* __restrict__ fin,
                                                                unsigned* __restrict__ hist, const int chain_passes,
                                                                const unsigned n_tiles) {
  constexpr int R = 1 << RB;
  constexpr int kCP = (RB == 8) ? kChainPasses : 1;      // (the chained sort runs 8-bit digits only)
  if (blockIdx.x == 0 && threadIdx.x == 0) {             // fix-up work-list length and arrival counter (rbx_segreduce.h)
    fin[0] = 0;
    fin[1] = 0;
    fin[2] = 0;
  }
  __shared__ KeyField sf[RBX_MAX_FIELDS];
  {
    const int words = n_cat * static_cast<int>(sizeof(KeyField) / 4);
    const int* src = reinterpret_cast<const int*>(&P);
    int* dst = reinterpret_cast<int*>(sf);
    for (int i = threadIdx.x; i < words; i += blockDim.x) dst[i] = src[i];
  }
  __shared__ unsigned cnt[kCP][R];
  for (int d = threadIdx.x; d < kCP * R; d += kSortThreads) (&cnt[0][0])[d] = 0;
  __syncthreads();
  int seg;
  unsigned tile0, tile_n;
  seg_of_tile(S, blockIdx.x, &seg, &tile0, &tile_n);
  const unsigned row0 = S.row0[seg];
  const int fp = S.first_pass[seg];
  unsigned* __restrict__ keys = (fp & 1) ? keys1 : keys0;
  unsigned* __restrict__ vals = (fp & 1) ? vals1 : vals0;
#pragma unroll
  for (int it = 0; it < kSortItems; ++it) {
    const unsigned off = it * kSortThreads + threadIdx.x;
    if (off >= tile_n) break;
    const unsigned j = tile0 + off;
    int lo = 0, hi = n_cat - 1;                          // last descriptor with lk_off <= j
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (sf[mid].lk_off <= j) lo = mid; else hi = mid - 1;
    }
    const KeyField& fd = sf[lo];
    const unsigned local = j - fd.lk_off;                // position inside the descriptor's index array (< nnz)
    const int bag = map[j];
    unsigned key = sentinel;
    if (bag >= 0) {
      const long long id = load_id(fd.ids, static_cast<long long>(local) * fd.stride_b, fd.dtype);
      if (id < 0 || id >= fd.vocab) {
        if (status != nullptr) atomicOr(status, kStatusBadId);
      } else {
        const bool id_pool = fd.pool == RBX_POOL_MEAN_ID || fd.pool == RBX_POOL_SUM_ID;
        if (id != fd.pad_id && !(id_pool && id == fd.mask_id)) key = fd.row_base + static_cast<unsigned>(id);
      }
    }
    keys[j] = key;
    if constexpr (POS) vals[j] = (static_cast<unsigned>(lo) << kLocalBits) | local;
    else vals[j] = (static_cast<unsigned>(lo) << kLocalBits) | static_cast<unsigned>(bag < 0 ? 0 : bag);
    if (chain_passes > 0) {
#pragma unroll
      for (int k = 0; k < kCP; ++k)
        if (fp + k < chain_passes) atomicAdd(&cnt[k][seg_digit<RB>(key, sentinel, row0, k * RB)], 1u);
    } else if (fp == 0) {
      atomicAdd(&cnt[0][seg_digit<RB>(key, sentinel, row0, 0)], 1u);
    }
  }
  if (chain_passes > 0) {
    // [pass][tile][digit] counts, [pass][tile] flags: the layout radix_scatter_kernel<RB, true> reads (rbx_embed_bwd.hip)
    __syncthreads();
    const size_t plane = static_cast<size_t>(n_tiles) * R;
    unsigned* flags = hist + 2 * plane * chain_passes;
    for (int k = 0; fp + k < chain_passes; ++k) {
      unsigned* h = hist + plane * (fp + k) + static_cast<size_t>(blockIdx.x) * R;
      for (int d = threadIdx.x; d < R; d += kSortThreads) h[d] = cnt[k < kCP ? k : 0][d];
      if (threadIdx.x == 0) flags[static_cast<size_t>(fp + k) * n_tiles + blockIdx.x] = 0u;
    }
    return;
  }
  if (fp != 0) return;
  __syncthreads();
  // histogram layout: segment, then digit, then tile of the segment (what the flat exclusive scan expects)
  const unsigned t_in = blockIdx.x - S.tile0[seg], nt = S.tile0[seg + 1] - S.tile0[seg];
  unsigned* h = hist + static_cast<size_t>(S.tile0[seg]) * R + t_in;
  for (int d = threadIdx.x; d < R; d += kSortThreads) h[static_cast<size_t>(d) * nt] = cnt[0][d];
}

// ---- host plan: the bags as seq_len = 1 fields of make_plan, descriptor i owning nnz_i lookups ----------------------
struct CsrPlan {
  BwdPlan p;
  BagPack bags;             // the descriptors that take part (grad != NULL), in the plan's order
  BagLookups lk;
  size_t off_map = 0, bytes = 0;
};

static int csr_plan(const rbx_bag_t* bags, int n, int64_t batch, const float* dout, int64_t stride_b, CsrPlan* c) {
  BagK all[RBX_MAX_BAGS];
  int rc = pack_bags(bags, n, batch, all);
  if (rc != RBX_OK) return rc;
  rbx_field_t fields[RBX_MAX_BAGS];
  unsigned long long lookups_of[RBX_MAX_BAGS];
  for (int i = 0; i < n; ++i) {
    const rbx_bag_t& g = bags[i];
    rbx_field_t& f = fields[i];
    f.ids = g.indices != nullptr ? g.indices : static_cast<const void*>(g.table);   // (nnz == 0: never read)
    f.table = g.table;
    f.grad = g.grad;
    f.ids_stride_b = g.indices_stride;
    f.ids_stride_l = 0;
    f.vocab = g.vocab;
    f.padding_idx = g.padding_idx;
    f.mask_id = g.mask_id;
    f.out_off = g.out_off;
    f.dim = g.dim;
    f.seq_len = 1;
    f.ids_dtype = g.indices_dtype;
    f.kind = RBX_FIELD_CATEGORICAL;
    // the sort of a max pool drops what the sort of RBX_POOL_SUM_ID drops (padding_idx, mask_id when set, ids out of range):
    // the padded path's plan is handed that pool and learns no new one
    f.pool = g.pool == RBX_POOL_MAX ? RBX_POOL_SUM_ID : g.pool;
    f.eps = g.eps;
    f.table_stride = 0;
    lookups_of[i] = static_cast<unsigned long long>(g.nnz);
  }
  rc = make_plan(fields, n, batch, dout, stride_b, &c->p, 0, lookups_of);
  if (rc != RBX_OK) return rc;
  int k = 0;
  for (int i = 0; i < n; ++i) {
    if (bags[i].grad == nullptr) continue;                // frozen: make_plan skipped it
    c->bags.f[k] = all[i];
    c->lk.lk_off[k] = c->p.keys.f[k].lk_off;
    ++k;
  }
  c->off_map = c->p.bytes;
  c->bytes = c->p.bytes + (static_cast<size_t>(c->p.n_lookups) * 4 + 255) / 256 * 256;
  return RBX_OK;
}

int csr_bwd_plan(const rbx_bag_t* bags, int n, int64_t batch, BwdPlan* p, size_t* bytes) {
  CsrPlan c;
  const int rc = csr_plan(bags, n, batch, nullptr, 0, &c);
  if (rc != RBX_OK) return rc;
  *p = c.p;
  *bytes = c.bytes;
  return RBX_OK;
}

template <int RB, bool POS = false>
static int launch_csr_keys(const CsrPlan& c, char* ws, int* status, hipStream_t s) {
  const BwdPlan& p = c.p;
  const bool chained = p.chained && RB == 8;
  hipLaunchKernelGGL((csr_keys_kernel<RB, POS>), dim3(p.n_tiles), dim3(kSortThreads), 0, s, p.keys, p.n_cat, p.segs, p.total_rows,
                     reinterpret_cast<const int*>(ws + c.off_map), reinterpret_cast<unsigned*>(ws + p.off_keys[0]),
                     reinterpret_cast<unsigned*>(ws + p.off_vals[0]), reinterpret_cast<unsigned*>(ws + p.off_keys[1]),
                     reinterpret_cast<unsigned*>(ws + p.off_vals[1]), status, reinterpret_cast<unsigned*>(ws + p.off_fin),
                     reinterpret_cast<unsigned*>(ws + p.off_hist), chained ? p.passes : 0, p.n_tiles);
  return check_launch("csr_keys_kernel");
}

// ---- the position-valued reduces -----------------------------------------------------------------------------------------
// What GenericPolicy (rbx_embed_bwd.hip) does around its fetch, for the two policies whose pairs name a position
// (csr_keys_kernel<RB, true>): no count, the factor as fetched, the old gradient row read when the call accumulates, one
// store per row.  `A` is the policy's Args; only Args and fetch are a policy's own.
struct BagPolicyBase {
  static constexpr bool kHasCount = false;
  template <class A>
  static __device__ __forceinline__ float weight(const A&, float w) { return w; }
  template <class A, class F>
  static __device__ __forceinline__ void prefetch(const A& a, const RedField& fd, unsigned row, int lane_g, F& pre) {
    if (a.accumulate) pre.add_from(fd.grad + static_cast<size_t>(row) * fd.dim, fd.dim, lane_g);
  }
  template <class A, class F>
  static __device__ __forceinline__ void prefetch_raw(const A& a, const RedField& fd, unsigned row, int lane_g, F& pre) {
    if (a.accumulate) pre.load_from(fd.grad + static_cast<size_t>(row) * fd.dim, fd.dim, lane_g);
  }
  template <class A, class F>
  static __device__ __forceinline__ void flush(const A&, const RedField& fd, unsigned row, const F& acc, float, const F& pre,
                                               int lane_g) {
    F out = acc;
    frag_add(out, pre);
    out.store_nt(fd.grad + static_cast<size_t>(row) * fd.dim, fd.dim, lane_g);
  }
};

// weighted reduce: a lookup contributes w[position] * dY[map[position], slot] -- the bag comes from the lookup -> bag map of
// the sort, the factor from the descriptor's weight array (NULL: 1)
struct WeightedBagPolicy : BagPolicyBase {
  struct Args {
    const float* dout;
    long long stride_b;
    const int* map;
    int accumulate;
    unsigned lk_off[RBX_MAX_BAGS];        // by descriptor index (RedField::slot)
    const float* w[RBX_MAX_BAGS];
  };
  template <class F>
  static __device__ __forceinline__ void fetch(const Args& a, const RedField& fd, unsigned pos, int lane_g, F& frag, float& w) {
    const int bag = a.map[a.lk_off[fd.slot] + pos];
    const float* wp = a.w[fd.slot];
    w = (wp != nullptr) ? wp[pos] : 1.0f;
    frag.load_from(a.dout + static_cast<long long>(bag) * a.stride_b + fd.out_off, fd.dim, lane_g);
  }
};

// max reduce: a lookup contributes dY[map[position], c] where argpos[that bag, c] names its position -- WeightedBagPolicy
// with a mask instead of a factor.  The mask is applied in place, right behind the two loads: a second
// per-lookup fragment for the argpos slice would hold U * NV * 4 more registers than RBX_REDUCE_WAVES leaves at the wide
// forms, and this reduce is on no measured step.  argpos is compared with the position and never used as an address: no
// content of that buffer makes a kernel read out of bounds.
struct MaxBagPolicy : BagPolicyBase {
  struct Args {
    const float* dout;
    long long stride_b;
    const int* argpos;
    long long arg_stride;
    const int* map;
    int accumulate;
    unsigned lk_off[RBX_MAX_BAGS];        // by descriptor index (RedField::slot)
  };
  template <int G, int NV, bool VEC>
  static __device__ __forceinline__ void fetch(const Args& a, const RedField& fd, unsigned pos, int lane_g, Frag<G, NV, VEC>& frag,
                                               float& w) {
    const int bag = a.map[a.lk_off[fd.slot] + pos];
    w = 1.0f;
    frag.load_from(a.dout + static_cast<long long>(bag) * a.stride_b + fd.out_off, fd.dim, lane_g);
    const int* __restrict__ arg = a.argpos + static_cast<long long>(bag) * a.arg_stride + fd.out_off;
    const int me = static_cast<int>(pos);
    constexpr int W = VEC ? 4 : 1;
#pragma unroll
    for (int u = 0; u < NV; ++u) {
      int e = (lane_g + u * G) * W;
      e = e < fd.dim ? e : fd.dim - W;                     // load_from's rule: lanes beyond dim re-read the last vector
      if constexpr (VEC) {
        const int4 t = *reinterpret_cast<const int4*>(arg + e);
        frag.a[u * 4 + 0] = t.x == me ? frag.a[u * 4 + 0] : 0.f;
        frag.a[u * 4 + 1] = t.y == me ? frag.a[u * 4 + 1] : 0.f;
        frag.a[u * 4 + 2] = t.z == me ? frag.a[u * 4 + 2] : 0.f;
        frag.a[u * 4 + 3] = t.w == me ? frag.a[u * 4 + 3] : 0.f;
      } else {
        frag.a[u] = arg[e] == me ? frag.a[u] : 0.f;
      }
    }
  }
};
// 16 floats per lane (D > 512): with 4 lookups in flight the masked fetch spilled 264 B per lane at RBX_REDUCE_WAVES; 2 fit
template <>
struct ReduceWideBatch<MaxBagPolicy> {
  static constexpr int of(int per_lane) { return per_lane > 8 ? 2 : 4; }
};
// the mask zeroes single elements: the lanes of a group disagree on whether a chunk's tail is zero
template <>
struct ReduceLaneZeros<MaxBagPolicy> {
  static constexpr bool value = true;
};

// the sort of both paths: map, pairs (POS: position-valued), radix passes
static int csr_sort(const rbx_bag_t* bags, int n_bags, int64_t batch, void* d_workspace, size_t workspace_bytes,
                    int* d_status, hipStream_t s, bool pos) {
  CsrPlan c;
  int rc = csr_plan(bags, n_bags, batch, nullptr, 0, &c);
  if (rc != RBX_OK) return rc;
  const BwdPlan& p = c.p;
  if (p.n_lookups == 0 || batch == 0) return RBX_OK;
  if (d_workspace == nullptr || workspace_bytes < c.bytes)
    return fail(RBX_ERR_WORKSPACE, "workspace %zu B < required %zu B", workspace_bytes, c.bytes);
  char* ws = static_cast<char*>(d_workspace);
  int* map = reinterpret_cast<int*>(ws + c.off_map);
  if (hipMemsetAsync(map, 0xFF, static_cast<size_t>(p.n_lookups) * 4, s) != hipSuccess)   // -1: outside every bag
    return fail(RBX_ERR_LAUNCH, "clearing the lookup -> bag map failed");
  long long bx = (batch + 15) / 16;
  if (bx > kCUs * 8) bx = kCUs * 8;
  hipLaunchKernelGGL(csr_bag_map_kernel, dim3(static_cast<unsigned>(bx), p.n_cat), dim3(256), 0, s, c.bags, c.lk,
                     static_cast<long long>(batch), map, d_status);
  rc = check_launch("csr_bag_map_kernel");
  if (rc != RBX_OK) return rc;
  switch (p.radix_bits) {
    case 8: rc = pos ? launch_csr_keys<8, true>(c, ws, d_status, s) : launch_csr_keys<8>(c, ws, d_status, s); break;
    case 10: rc = pos ? launch_csr_keys<10, true>(c, ws, d_status, s) : launch_csr_keys<10>(c, ws, d_status, s); break;
    default: rc = pos ? launch_csr_keys<11, true>(c, ws, d_status, s) : launch_csr_keys<11>(c, ws, d_status, s); break;
  }
  if (rc != RBX_OK) return rc;
  return run_sort_passes(p, ws, s);
}

// a mean pool's backward needs the row scale the unweighted forward leaves; the weighted entry points carry none
static int check_no_trained_mean(const rbx_bag_t* bags, int n, const char* who) {
  for (int i = 0; bags != nullptr && i < n; ++i)
    if (bags[i].grad != nullptr && (bags[i].pool == RBX_POOL_MEAN_ID || bags[i].pool == RBX_POOL_MEAN_VALUE))
      return fail(RBX_ERR_UNSUPPORTED, "%s: bag %d is a mean pool with a gradient; its backward goes through rbx_embed_csr_sort / "
                  "rbx_embed_csr_bwd (d_row_scale)", who, i);
  return RBX_OK;
}

// ---- the long-bag form, host side and finish ---------------------------------------------------------------------------
// A wave per recorded bag: the partial rows of its segments are summed in ascending slot order, the mean pools get
// 1 / (count + eps) over the partial counts summed the same way, and the row and row_scale[slot * B + bag] go where the
// lane-group kernel would have put them.  P holds every descriptor of the call by index (LongRec::desc).
__global__ __launch_bounds__(256) void csr_long_finish_kernel(const BagPack P, const int F, const long long B,
                                                              float* __restrict__ out, const long long stride_b,
                                                              float* __restrict__ row_scale, const LongArgs LA) {
  int n_long;
  long long n_segs;
  long_counts(LA, &n_long, &n_segs);
  const int lane = threadIdx.x & 63;
  for (long long r = static_cast<long long>(blockIdx.x) * 4 + threadIdx.x / 64; r < n_long;
       r += static_cast<long long>(gridDim.x) * 4) {
    const LongRec rec = LA.recs[r];
    if (rec.end <= rec.begin || static_cast<unsigned>(rec.desc) >= static_cast<unsigned>(F)) continue;   // refused: walked in place
    const long long nseg = (static_cast<long long>(rec.end) - rec.begin + kSeg - 1) / kSeg;
    if (rec.seg0 < 0 || rec.seg0 + nseg > n_segs || rec.bag < 0 || rec.bag >= B) continue;              // (long_append checked)
    const BagK& fd = P.f[rec.desc];
    const bool mean = fd.pool == RBX_POOL_MEAN_VALUE || fd.pool == RBX_POOL_MEAN_ID;
    float inv = 1.0f;
    if (mean) {
      float count = 0.f;
      for (long long j = 0; j < nseg; ++j) count += LA.pcnt[rec.seg0 + j];
      inv = 1.0f / (count + fd.eps);
      if (row_scale != nullptr && lane == 0) row_scale[static_cast<long long>(fd.slot) * B + rec.bag] = inv;
    }
    float* dst = out + rec.bag * stride_b + fd.out_off;
    const float* src = LA.part + static_cast<long long>(rec.seg0) * LA.pstride;
    for (int d = lane; d < fd.dim; d += 64) {
      float a = 0.f;
      for (long long j = 0; j < nseg; ++j) a += src[j * LA.pstride + d];
      dst[d] = mean ? a * inv : a;
    }
  }
}

// The max pool's finish, a wave per recorded bag: the maximum over the partial rows of its segments in ascending slot order
// under strict > -- a later segment holds higher positions, so on equal values the earlier one keeps the element -- and a
// partial with position -1 (no usable id in that segment) is skipped.  Exact: the bits of the lane-group walk.
__global__ __launch_bounds__(256) void csr_long_max_finish_kernel(const BagPack P, const int F, const long long B,
                                                                  float* __restrict__ out, const long long stride_b,
                                                                  int* __restrict__ argpos, const long long arg_stride,
                                                                  const int* __restrict__ parg, const LongArgs LA) {
  int n_long;
  long long n_segs;
  long_counts(LA, &n_long, &n_segs);
  const int lane = threadIdx.x & 63;
  for (long long r = static_cast<long long>(blockIdx.x) * 4 + threadIdx.x / 64; r < n_long;
       r += static_cast<long long>(gridDim.x) * 4) {
    const LongRec rec = LA.recs[r];
    if (rec.end <= rec.begin || static_cast<unsigned>(rec.desc) >= static_cast<unsigned>(F)) continue;   // refused: walked in place
    const long long nseg = (static_cast<long long>(rec.end) - rec.begin + kSeg - 1) / kSeg;
    if (rec.seg0 < 0 || rec.seg0 + nseg > n_segs || rec.bag < 0 || rec.bag >= B) continue;              // (long_append checked)
    const BagK& fd = P.f[rec.desc];
    float* dst = out + rec.bag * stride_b + fd.out_off;
    int* adst = argpos + rec.bag * arg_stride + fd.out_off;
    const float* src = LA.part + static_cast<long long>(rec.seg0) * LA.pstride;
    const int* asrc = parg + static_cast<long long>(rec.seg0) * LA.pstride;
    for (int d = lane; d < fd.dim; d += 64) {
      float best = 0.f;
      int at = -1;
      for (long long j = 0; j < nseg; ++j) {
        const int p = asrc[j * LA.pstride + d];
        const float v = src[j * LA.pstride + d];
        if (p >= 0 && (at < 0 || v > best)) {
          best = v;
          at = p;
        }
      }
      dst[d] = best;
      adst[d] = at;
    }
  }
}

// Workspace of the long-bag calls: [header 256 B | records | partial rows | partial counts], sized from static values.
// Well-formed offsets give at most nnz_i / T bags of >= T ids in descriptor i (and at most `batch`), and their segments
// number sum(ceil(L / S)) <= nnz_i / S + that many.
struct LongPlan {
  int T = 0, cap_bags = 0, cap_segs = 0, pstride = 4;
  size_t off_recs = 0, off_part = 0, off_cnt = 0, bytes = 0;
};
constexpr size_t kLongHeader = 256;

static int long_plan(const rbx_bag_t* bags, int n, int64_t batch, int64_t threshold, LongPlan* lp) {
  int rc = check_sizes(bags, n, batch, -1);
  if (rc != RBX_OK) return rc;
  if (threshold < 0) return fail(RBX_ERR_INVALID, "negative long_threshold");
  long long cap_bags = 0, cap_segs = 0;
  int dim = 1;
  for (int i = 0; i < n; ++i) {
    const rbx_bag_t& g = bags[i];
    rc = check_sizes(bags, n, batch, i);
    if (rc != RBX_OK) return rc;
    if (g.dim > dim) dim = g.dim;
    if (threshold == 0) continue;
    const long long most = g.nnz / threshold < batch ? g.nnz / threshold : batch;
    cap_bags += most;
    cap_segs += g.nnz / kSeg + most;
  }
  if (cap_bags == 0) cap_segs = 0;
  lp->T = threshold > INT_MAX ? INT_MAX : static_cast<int>(threshold);
  lp->cap_bags = static_cast<int>(cap_bags);             // <= 32 * 2^26 / T
  lp->cap_segs = static_cast<int>(cap_segs);             // <= 32 * 2^26 / 256 + cap_bags
  lp->pstride = (dim + 3) / 4 * 4;
  auto up = [](size_t v) { return (v + 255) / 256 * 256; };
  lp->off_recs = kLongHeader;
  lp->off_part = lp->off_recs + up(static_cast<size_t>(cap_bags) * sizeof(LongRec));
  lp->off_cnt = lp->off_part + up(static_cast<size_t>(cap_segs) * lp->pstride * 4);
  lp->bytes = lp->off_cnt + up(static_cast<size_t>(cap_segs) * 4);
  return RBX_OK;
}

static LongArgs long_args(const LongPlan& lp, void* ws) {
  char* base = static_cast<char*>(ws);
  LongArgs la;
  la.hdr = reinterpret_cast<unsigned long long*>(base);
  la.recs = reinterpret_cast<LongRec*>(base + lp.off_recs);
  la.part = reinterpret_cast<float*>(base + lp.off_part);
  la.pcnt = reinterpret_cast<float*>(base + lp.off_cnt);
  la.T = lp.T;
  la.cap_bags = lp.cap_bags;
  la.cap_segs = lp.cap_segs;
  la.pstride = lp.pstride;
  la.cls = 0;
  return la;
}

// plan + workspace check + the memset node that clears the header; *on: some bag of the call can take the long form
static int long_begin(const rbx_bag_t* bags, int n, int64_t batch, int64_t threshold, void* ws, size_t ws_bytes, hipStream_t s,
                      LongPlan* lp, bool* on) {
  int rc = long_plan(bags, n, batch, threshold, lp);
  if (rc != RBX_OK) return rc;
  if (ws == nullptr || ws_bytes < lp->bytes)
    return fail(RBX_ERR_WORKSPACE, "workspace %zu B < required %zu B", ws == nullptr ? size_t(0) : ws_bytes, lp->bytes);
  if (hipMemsetAsync(ws, 0, kLongHeader, s) != hipSuccess) return fail(RBX_ERR_LAUNCH, "clearing the long-bag header failed");
  *on = lp->cap_bags > 0 && batch > 0;
  return RBX_OK;
}

// ---- host side of the bag walk: launch classes, the forward driver, the weight-gradient driver -------------------------
// The descriptors of a call sorted into launch classes: class k = (float4 ? 0 : 1) + (2 when the descriptor walks with a
// per-lookup array of the forward: its weights).  `per` is that array per descriptor (NULL: none); with `only_per` a
// descriptor without one takes no part and the classes are 0 / 1 (the weight gradient).  Every dim is checked here, in
// front of the first memset or launch, so a refused call writes nothing.
template <class T>
struct BagClasses {
  BagPack pack[4];
  BagPtrs<T> ptr[4], whole = {};    // the arrays of a class in pack order; of the whole call by descriptor index
  int cnt[4] = {0, 0, 0, 0}, units[4] = {1, 1, 1, 1};
};

template <class T>
static int classify_bags(const rbx_bag_t* bags, const BagPack& all, int n, const float* rows, int64_t stride_b, T* const* per,
                         bool only_per, BagClasses<T>* c) {
  for (int i = 0; i < n; ++i) {
    T* const p = per != nullptr ? per[i] : nullptr;
    if (only_per && p == nullptr) continue;
    const bool vec = bag_vec_ok(bags[i], rows, stride_b);
    const int k = (vec ? 0 : 1) + (p != nullptr && !only_per ? 2 : 0);
    c->ptr[k].p[c->cnt[k]] = p;
    c->whole.p[i] = p;
    c->pack[k].f[c->cnt[k]++] = all.f[i];
    const int u = vec ? bags[i].dim / 4 : bags[i].dim;
    if (u > c->units[k]) c->units[k] = u;
  }
  for (int k = 0; k < 4; ++k)
    if (c->cnt[k] > 0 && pow2_ceil(c->units[k]) > 256)
      return fail(RBX_ERR_UNSUPPORTED, "embedding dim too large for one lane group (%s units=%d)", k % 2 == 0 ? "float4" : "scalar",
                  c->units[k]);
  return RBX_OK;
}

// The launch sequence of every walk, in its fixed order: the lane-group launches of the classes in ascending order (kWalk,
// or kHandOff when `on`: some bag of the call can take the long form, and these launches fill the record list); with `on`
// the classes' segment launches, over every descriptor of the call by index (LongRec::desc), and then `finish`.
// launch(k, mode, pack, count, arrays, la) picks the op of class k and builds its Args.
template <class T, class Launch, class Finish>
static int walk_phases(const BagClasses<T>& c, const BagPack& all, int n_bags, LongArgs la, bool on, Launch launch, Finish finish) {
  for (int phase = 0; phase < (on ? 2 : 1); ++phase) {
    const int mode = phase == 1 ? kSegments : on ? kHandOff : kWalk;
    for (int k = 0; k < 4; ++k) {
      if (c.cnt[k] == 0) continue;
      la.cls = k;
      const int rc = mode == kSegments ? launch(k, mode, all, n_bags, c.whole, la) : launch(k, mode, c.pack[k], c.cnt[k], c.ptr[k], la);
      if (rc != RBX_OK) return rc;
    }
  }
  return on ? finish(la) : RBX_OK;
}

// the finish kernels' grid: a wave per record, grid-striding beyond two workgroups per CU
static dim3 finish_grid(const LongPlan& lp) {
  const long long fb = (static_cast<long long>(lp.cap_bags) + 3) / 4;
  return dim3(static_cast<unsigned>(fb > kCUs * 2 ? kCUs * 2 : fb));
}

// The four forward entry points.  weighted_call: d_weights is looked at (NULL entries walk unweighted, without a row
// scale: the caller passes none); has_long: the `_long` calls, whose bags of >= threshold ids go out in segments.
static int csr_forward(const rbx_bag_t* bags, int n_bags, int64_t batch, bool has_long, int64_t threshold,
                       const float* const* d_weights, bool weighted_call, float* d_out, int64_t out_stride_b, float* d_row_scale,
                       void* d_workspace, size_t workspace_bytes, int* d_status, hipStream_t s) {
  BagPack all;
  int rc = pack_bags(bags, n_bags, batch, all.f);
  if (rc != RBX_OK) return rc;
  rc = check_no_max(bags, n_bags, "the sum / mean forward");
  if (rc != RBX_OK) return rc;
  if (weighted_call) {
    rc = check_weighted_pools(bags, n_bags, reinterpret_cast<const void* const*>(d_weights), "a weight array");
    if (rc != RBX_OK) return rc;
  }
  if (!has_long && batch == 0) return RBX_OK;
  if (batch > 0 && d_out == nullptr) return fail(RBX_ERR_INVALID, "d_out is NULL");
  BagClasses<const float> c;
  rc = classify_bags(bags, all, n_bags, d_out, out_stride_b, d_weights, false, &c);
  if (rc != RBX_OK) return rc;
  LongPlan lp;
  LongArgs la = {};
  bool on = false;
  if (has_long) {
    rc = long_begin(bags, n_bags, batch, threshold, d_workspace, workspace_bytes, s, &lp, &on);
    if (rc != RBX_OK) return rc;
    if (batch == 0) return RBX_OK;
    la = long_args(lp, d_workspace);
  }
  return walk_phases(
      c, all, n_bags, la, on,
      [&](int k, int mode, const BagPack& pack, int cnt, const BagWeights& w, const LongArgs& la) {
        if (k < 2)                                          // (a segment stores no row scale: the finish scales)
          return bag_walk<PoolOp>(k % 2 == 0, mode, c.units[k], pack, cnt, batch,
                                  {d_out, out_stride_b, mode == kSegments ? nullptr : d_row_scale}, d_status, s, la);
        return bag_walk<WeightedPoolOp>(k % 2 == 0, mode, c.units[k], pack, cnt, batch, {w, d_out, out_stride_b}, d_status, s, la);
      },
      [&](const LongArgs& la) {
        hipLaunchKernelGGL(csr_long_finish_kernel, finish_grid(lp), dim3(256), 0, s, all, n_bags, static_cast<long long>(batch),
                           d_out, static_cast<long long>(out_stride_b), d_row_scale, la);
        return check_launch("csr_long_finish_kernel");
      });
}

// Both weight-gradient entry points; a descriptor takes part when it has somewhere to put its gradient.
static int csr_weight_grad(const rbx_bag_t* bags, int n_bags, int64_t batch, bool has_long, int64_t threshold, const float* d_dout,
                           int64_t out_stride_b, float* const* d_dweights, void* d_workspace, size_t workspace_bytes,
                           int* d_status, hipStream_t s) {
  BagPack all;
  int rc = pack_bags(bags, n_bags, batch, all.f);
  if (rc != RBX_OK) return rc;
  rc = check_no_max(bags, n_bags, "the weight gradient");
  if (rc != RBX_OK) return rc;
  if (d_dweights == nullptr) return fail(RBX_ERR_INVALID, "d_dweights is NULL");
  rc = check_weighted_pools(bags, n_bags, reinterpret_cast<const void* const*>(d_dweights), "a weight gradient");
  if (rc != RBX_OK) return rc;
  if (batch > 0 && d_dout == nullptr) return fail(RBX_ERR_INVALID, "d_dout is NULL");
  BagClasses<float> c;
  rc = classify_bags(bags, all, n_bags, d_dout, out_stride_b, d_dweights, true, &c);
  if (rc != RBX_OK) return rc;
  LongPlan lp;
  LongArgs la = {};
  bool on = false;
  if (has_long) {
    rc = long_begin(bags, n_bags, batch, threshold, d_workspace, workspace_bytes, s, &lp, &on);
    if (rc != RBX_OK) return rc;
    la = long_args(lp, d_workspace);
  }
  // dw is fully defined after the call: everything the kernel does not write (masked and out-of-range ids, positions
  // outside every bag, a batch of zero bags) is cleared here
  for (int i = 0; i < n_bags; ++i)
    if (d_dweights[i] != nullptr && bags[i].nnz > 0 &&
        hipMemsetAsync(d_dweights[i], 0, static_cast<size_t>(bags[i].nnz) * 4, s) != hipSuccess)
      return fail(RBX_ERR_LAUNCH, "clearing a weight gradient failed");
  if (batch == 0) return RBX_OK;
  return walk_phases(
      c, all, n_bags, la, on,
      [&](int k, int mode, const BagPack& pack, int cnt, const BagWeightGrads& dw, const LongArgs& la) {
        return bag_walk<WeightGradOp>(k == 0, mode, c.units[k], pack, cnt, batch, {dw, d_dout, out_stride_b}, d_status, s, la);
      },
      [](const LongArgs&) { return RBX_OK; });              // the same segment tasks, nothing to combine
}

// The max forward.  Its workspace is the long workspace with one int32 partial argpos row per segment slot behind it.
static size_t max_workspace_bytes(const LongPlan& lp) {
  return lp.bytes + (static_cast<size_t>(lp.cap_segs) * lp.pstride * 4 + 255) / 256 * 256;
}

static int csr_forward_max(const rbx_bag_t* bags, int n_bags, int64_t batch, int64_t threshold, float* d_out, int64_t out_stride_b,
                           int* d_argpos, int64_t arg_stride_b, void* d_workspace, size_t workspace_bytes, int* d_status,
                           hipStream_t s) {
  BagPack all;
  int rc = pack_bags(bags, n_bags, batch, all.f);
  if (rc != RBX_OK) return rc;
  rc = check_all_max(bags, n_bags, "rbx_embed_csr_fwd_max");
  if (rc != RBX_OK) return rc;
  LongPlan lp;
  rc = long_plan(bags, n_bags, batch, threshold, &lp);
  if (rc != RBX_OK) return rc;
  if (batch == 0) return RBX_OK;
  if (d_out == nullptr) return fail(RBX_ERR_INVALID, "d_out is NULL");
  if (d_argpos == nullptr) return fail(RBX_ERR_INVALID, "d_argpos is NULL");
  BagClasses<const float> c;                              // two launch classes here: float4 and scalar
  rc = classify_bags<const float>(bags, all, n_bags, d_out, out_stride_b, nullptr, false, &c);
  if (rc != RBX_OK) return rc;
  LongArgs la = {};
  bool on = false;
  int* parg = nullptr;
  if (threshold > 0) {                                    // 0: no hand-off and no workspace
    const size_t need = max_workspace_bytes(lp);
    if (d_workspace == nullptr || workspace_bytes < need)
      return fail(RBX_ERR_WORKSPACE, "workspace %zu B < required %zu B", d_workspace == nullptr ? size_t(0) : workspace_bytes, need);
    rc = long_begin(bags, n_bags, batch, threshold, d_workspace, workspace_bytes, s, &lp, &on);
    if (rc != RBX_OK) return rc;
    la = long_args(lp, d_workspace);
    parg = reinterpret_cast<int*>(static_cast<char*>(d_workspace) + lp.bytes);
  }
  const int arg_vec = (arg_stride_b % 4 == 0 && (reinterpret_cast<uintptr_t>(d_argpos) & 15) == 0) ? 1 : 0;
  const MaxPoolOp::Args args = {d_out, out_stride_b, d_argpos, arg_stride_b, parg, arg_vec};
  return walk_phases(
      c, all, n_bags, la, on,
      [&](int k, int mode, const BagPack& pack, int cnt, const BagWeights&, const LongArgs& la) {
        return bag_walk<MaxPoolOp>(k == 0, mode, c.units[k], pack, cnt, batch, args, d_status, s, la);
      },
      [&](const LongArgs& la) {
        hipLaunchKernelGGL(csr_long_max_finish_kernel, finish_grid(lp), dim3(256), 0, s, all, n_bags,
                           static_cast<long long>(batch), d_out, static_cast<long long>(out_stride_b), d_argpos,
                           static_cast<long long>(arg_stride_b), parg, la);
        return check_launch("csr_long_max_finish_kernel");
      });
}

// The epilogue of the two position-valued reduces (rbx_embed_csr_bwd_weighted, rbx_embed_csr_bwd_max), behind their NULL
// checks: the plan, `pools_ok()` (which pools the call takes), the workspace test, the Args fields every such policy has,
// then `fill(p, &args, &vec)` for the policy's own fields and its say on the float4 form.
template <class Policy, class Check, class Fill>
static int position_reduce(const rbx_bag_t* bags, int n_bags, int64_t batch, const float* d_dout, int64_t out_stride_b,
                           int accumulate, void* d_workspace, size_t workspace_bytes, hipStream_t s, Check pools_ok, Fill fill) {
  CsrPlan c;
  int rc = csr_plan(bags, n_bags, batch, d_dout, out_stride_b, &c);
  if (rc != RBX_OK) return rc;
  rc = pools_ok();
  if (rc != RBX_OK) return rc;
  const BwdPlan& p = c.p;
  if (p.n_lookups == 0 || batch == 0) return RBX_OK;
  if (d_workspace == nullptr || workspace_bytes < c.bytes)
    return fail(RBX_ERR_WORKSPACE, "workspace %zu B < required %zu B", workspace_bytes, c.bytes);
  char* ws = static_cast<char*>(d_workspace);
  typename Policy::Args args = {};
  args.dout = d_dout;
  args.stride_b = out_stride_b;
  args.map = reinterpret_cast<const int*>(ws + c.off_map);
  args.accumulate = accumulate;
  for (int k = 0; k < p.n_cat; ++k) args.lk_off[p.red.f[k].slot] = p.keys.f[k].lk_off;   // by the descriptor's index in `bags`
  bool vec = p.vec;
  rc = fill(p, &args, &vec);
  if (rc != RBX_OK) return rc;
  const int cur = p.passes & 1;
  const unsigned* keys = reinterpret_cast<const unsigned*>(ws + p.off_keys[cur]);
  const unsigned* vals = reinterpret_cast<const unsigned*>(ws + p.off_vals[cur]);
  return vec ? dispatch_reduce<Policy, true>(p, args, keys, vals, ws, s) : dispatch_reduce<Policy, false>(p, args, keys, vals, ws, s);
}

}  // namespace rbx

extern "C" int rbx_embed_csr_fwd(const rbx_bag_t* bags, int32_t n_bags, int64_t batch, float* d_out, int64_t out_stride_b,
                                 float* d_row_scale, int32_t* d_status, void* stream) {
  return rbx::csr_forward(bags, n_bags, batch, false, 0, nullptr, false, d_out, out_stride_b, d_row_scale, nullptr, 0, d_status,
                          rbx::as_stream(stream));
}

extern "C" size_t rbx_embed_csr_bwd_workspace_size(const rbx_bag_t* bags, int32_t n_bags, int64_t batch) {
  rbx::CsrPlan c;
  if (rbx::csr_plan(bags, n_bags, batch, nullptr, 0, &c) != RBX_OK) return 0;
  return c.bytes;
}

extern "C" int rbx_embed_csr_sort(const rbx_bag_t* bags, int32_t n_bags, int64_t batch, void* d_workspace,
                                  size_t workspace_bytes, int32_t* d_status, void* stream) {
  return rbx::csr_sort(bags, n_bags, batch, d_workspace, workspace_bytes, d_status, rbx::as_stream(stream), false);
}

extern "C" int rbx_embed_csr_bwd(const rbx_bag_t* bags, int32_t n_bags, int64_t batch, const float* d_dout,
                                 int64_t out_stride_b, const float* d_row_scale, int32_t accumulate, void* d_workspace,
                                 size_t workspace_bytes, void* stream) {
  using namespace rbx;
  if (d_dout == nullptr) return fail(RBX_ERR_INVALID, "d_dout is NULL");
  CsrPlan c;
  int rc = csr_plan(bags, n_bags, batch, d_dout, out_stride_b, &c);
  if (rc != RBX_OK) return rc;
  rc = check_no_max(bags, n_bags, "rbx_embed_csr_bwd");
  if (rc != RBX_OK) return rc;
  if (c.p.n_lookups == 0 || batch == 0) return RBX_OK;
  if (d_workspace == nullptr || workspace_bytes < c.bytes)
    return fail(RBX_ERR_WORKSPACE, "workspace %zu B < required %zu B", workspace_bytes, c.bytes);
  return generic_reduce(c.p, d_dout, out_stride_b, nullptr, d_row_scale, batch, accumulate, static_cast<char*>(d_workspace),
                        as_stream(stream));
}

// The rows the previous rbx_embed_csr_bwd[_weighted] over this workspace stored: the run heads of its sorted pairs (either
// sort: keys and plan slots only are read).
extern "C" int rbx_embed_csr_rezero(const rbx_bag_t* bags, int32_t n_bags, int64_t batch, void* d_workspace,
                                    size_t workspace_bytes, void* stream) {
  using namespace rbx;
  CsrPlan c;
  int rc = csr_plan(bags, n_bags, batch, nullptr, 0, &c);
  if (rc != RBX_OK) return rc;
  if (c.p.n_lookups == 0 || batch == 0) return RBX_OK;
  if (d_workspace == nullptr || workspace_bytes < c.bytes)
    return fail(RBX_ERR_WORKSPACE, "workspace %zu B < required %zu B", d_workspace == nullptr ? size_t(0) : workspace_bytes, c.bytes);
  return launch_rezero(c.p, static_cast<const char*>(d_workspace), as_stream(stream));
}

// ---- per-sample weights ----------------------------------------------------------------------------------------------
extern "C" int rbx_embed_csr_fwd_weighted(const rbx_bag_t* bags, int32_t n_bags, int64_t batch, const float* const* d_weights,
                                          float* d_out, int64_t out_stride_b, int32_t* d_status, void* stream) {
  return rbx::csr_forward(bags, n_bags, batch, false, 0, d_weights, true, d_out, out_stride_b, nullptr, nullptr, 0, d_status,
                          rbx::as_stream(stream));
}

extern "C" int rbx_embed_csr_sort_weighted(const rbx_bag_t* bags, int32_t n_bags, int64_t batch, void* d_workspace,
                                           size_t workspace_bytes, int32_t* d_status, void* stream) {
  int rc = rbx::check_no_trained_mean(bags, n_bags, "rbx_embed_csr_sort_weighted");
  if (rc != RBX_OK) return rc;
  return rbx::csr_sort(bags, n_bags, batch, d_workspace, workspace_bytes, d_status, rbx::as_stream(stream), true);
}

extern "C" int rbx_embed_csr_bwd_weighted(const rbx_bag_t* bags, int32_t n_bags, int64_t batch, const float* const* d_weights,
                                          const float* d_dout, int64_t out_stride_b, int32_t accumulate, void* d_workspace,
                                          size_t workspace_bytes, void* stream) {
  using namespace rbx;
  if (d_dout == nullptr) return fail(RBX_ERR_INVALID, "d_dout is NULL");
  const int rc = check_no_trained_mean(bags, n_bags, "rbx_embed_csr_bwd_weighted");
  if (rc != RBX_OK) return rc;
  return position_reduce<WeightedBagPolicy>(
      bags, n_bags, batch, d_dout, out_stride_b, accumulate, d_workspace, workspace_bytes, as_stream(stream),
      [&] {
        const int rc = check_no_max(bags, n_bags, "rbx_embed_csr_bwd_weighted");
        if (rc != RBX_OK) return rc;
        return check_weighted_pools(bags, n_bags, reinterpret_cast<const void* const*>(d_weights), "a weight array");
      },
      [&](const BwdPlan& p, WeightedBagPolicy::Args* args, bool*) {
        for (int k = 0; d_weights != nullptr && k < p.n_cat; ++k) args->w[p.red.f[k].slot] = d_weights[p.red.f[k].slot];
        return RBX_OK;
      });
}

extern "C" int rbx_embed_csr_weight_grad(const rbx_bag_t* bags, int32_t n_bags, int64_t batch, const float* d_dout,
                                         int64_t out_stride_b, float* const* d_dweights, int32_t* d_status, void* stream) {
  return rbx::csr_weight_grad(bags, n_bags, batch, false, 0, d_dout, out_stride_b, d_dweights, nullptr, 0, d_status,
                              rbx::as_stream(stream));
}

// ---- the long-bag form (see LongArgs) ----------------------------------------------------------------------------------
extern "C" size_t rbx_embed_csr_fwd_long_workspace_size(const rbx_bag_t* bags, int32_t n_bags, int64_t batch,
                                                        int64_t long_threshold) {
  rbx::LongPlan lp;
  if (rbx::long_plan(bags, n_bags, batch, long_threshold, &lp) != RBX_OK) return 0;
  return lp.bytes;
}

extern "C" int rbx_embed_csr_fwd_long(const rbx_bag_t* bags, int32_t n_bags, int64_t batch, int64_t long_threshold, float* d_out,
                                      int64_t out_stride_b, float* d_row_scale, void* d_workspace, size_t workspace_bytes,
                                      int32_t* d_status, void* stream) {
  return rbx::csr_forward(bags, n_bags, batch, true, long_threshold, nullptr, false, d_out, out_stride_b, d_row_scale, d_workspace,
                          workspace_bytes, d_status, rbx::as_stream(stream));
}

extern "C" int rbx_embed_csr_fwd_weighted_long(const rbx_bag_t* bags, int32_t n_bags, int64_t batch, int64_t long_threshold,
                                               const float* const* d_weights, float* d_out, int64_t out_stride_b,
                                               void* d_workspace, size_t workspace_bytes, int32_t* d_status, void* stream) {
  return rbx::csr_forward(bags, n_bags, batch, true, long_threshold, d_weights, true, d_out, out_stride_b, nullptr, d_workspace,
                          workspace_bytes, d_status, rbx::as_stream(stream));
}

extern "C" int rbx_embed_csr_weight_grad_long(const rbx_bag_t* bags, int32_t n_bags, int64_t batch, int64_t long_threshold,
                                              const float* d_dout, int64_t out_stride_b, float* const* d_dweights,
                                              void* d_workspace, size_t workspace_bytes, int32_t* d_status, void* stream) {
  return rbx::csr_weight_grad(bags, n_bags, batch, true, long_threshold, d_dout, out_stride_b, d_dweights, d_workspace,
                              workspace_bytes, d_status, rbx::as_stream(stream));
}

// ---- the max pool (see MaxPoolOp, MaxBagPolicy) --------------------------------------------------------------------------
extern "C" size_t rbx_embed_csr_fwd_max_workspace_size(const rbx_bag_t* bags, int32_t n_bags, int64_t batch,
                                                       int64_t long_threshold) {
  rbx::LongPlan lp;
  if (rbx::long_plan(bags, n_bags, batch, long_threshold, &lp) != RBX_OK) return 0;
  return rbx::max_workspace_bytes(lp);
}

extern "C" int rbx_embed_csr_fwd_max(const rbx_bag_t* bags, int32_t n_bags, int64_t batch, int64_t long_threshold, float* d_out,
                                     int64_t out_stride_b, int32_t* d_argpos, int64_t arg_stride_b, void* d_workspace,
                                     size_t workspace_bytes, int32_t* d_status, void* stream) {
  return rbx::csr_forward_max(bags, n_bags, batch, long_threshold, d_out, out_stride_b, d_argpos, arg_stride_b, d_workspace,
                              workspace_bytes, d_status, rbx::as_stream(stream));
}

extern "C" int rbx_embed_csr_bwd_max(const rbx_bag_t* bags, int32_t n_bags, int64_t batch, const float* d_dout,
                                     int64_t out_stride_b, const int32_t* d_argpos, int64_t arg_stride_b, int32_t accumulate,
                                     void* d_workspace, size_t workspace_bytes, void* stream) {
  using namespace rbx;
  if (d_dout == nullptr) return fail(RBX_ERR_INVALID, "d_dout is NULL");
  if (d_argpos == nullptr) return fail(RBX_ERR_INVALID, "d_argpos is NULL");
  return position_reduce<MaxBagPolicy>(
      bags, n_bags, batch, d_dout, out_stride_b, accumulate, d_workspace, workspace_bytes, as_stream(stream),
      [&] { return check_all_max(bags, n_bags, "rbx_embed_csr_bwd_max"); },
      [&](const BwdPlan& p, MaxBagPolicy::Args* args, bool* vec) -> int {
        args->argpos = d_argpos;
        args->arg_stride = arg_stride_b;
        // the float4 form reads argpos in 16-byte vectors as well
        *vec = p.vec && arg_stride_b % 4 == 0 && (reinterpret_cast<uintptr_t>(d_argpos) & 15) == 0;
        if (!*vec && pow2_ceil(p.max_dim) > 256)
          return fail(RBX_ERR_UNSUPPORTED, "embedding dim %d too large for one lane group (scalar units: d_argpos is not 16-byte "
                      "aligned or arg_stride_b no multiple of 4)", p.max_dim);
        return RBX_OK;
      });
}
