// rbx_ffm.hip -- field-aware FM: gather and cross in one pass, forward and backward (gfx950).
//
// Reference behaviour replaced: third_party/rechub/models/ranking/deepffm.py (DeepFFM / FatDeepFFM) with the FFM layer of
// basic/layers.py:651-680.  Field i owns an nn.Embedding of vocab_i * F rows; id x names the F consecutive rows
// x*F .. x*F+F-1 (one [F*D] block).  The reference gathers all of them into [B, F, F, D], slices it P = F(F-1)/2 times
// and stacks the products; autograd keeps that tensor and makes another one as its gradient.  Every gathered row
// E[b,i,j] = table_i[x_i(b)*F + j] is used by exactly ONE pair, so here nothing is staged:
//   forward   out[b, p(i,j), :] = E[b,i,j] * E[b,j,i]   (i < j, i outer)      -- one launch, reads F(F-1) rows, writes P
//   backward  dE[b,i,j] = dout[b, p(i,j), :] * E[b,j,i] is formed inside the fetch of the sorted, segmented reduce of
//             rbx_segreduce.h: table i is viewed as [vocab_i / F, F*D], the (block, sample) pairs are sorted by the radix
//             machinery of rbx_embed_bwd.hip as they are, and the policy below builds a lane's slice of the F*D-wide
//             contribution of (block x of table i, sample b) from dout and the partner rows.  No float atomics.
#include "rbx_segreduce.h"

namespace rbx {

struct FfmField {            // 32 B
  const void* ids;
  const float* table;
  long long stride_b;
  int nblocks;               // vocab / F: ids in [0, nblocks) name a whole block
  int dtype;
};
struct FfmPack { FfmField f[RBX_MAX_FIELDS]; };

constexpr int kFfmMaxPairs = RBX_MAX_FIELDS * (RBX_MAX_FIELDS - 1) / 2;

// ---- forward -----------------------------------------------------------------------------------------------------
// A wavefront task is `spw` = 64 / F consecutive samples: lane l fetches the id of (sample l / F, field l % F) once, and
// every lane group then takes the ids of its pair by shuffle.  Units of a sample are walked in output order -- pair p, then
// the float4 inside the row -- so that neighbouring lanes share i and walk j: the reads of table i's block and the stores
// are contiguous, the partner rows table_j[x_j*F + i] are the scattered 4*D-byte reads.  An id outside [0, nblocks) reads
// as a zero block (addresses are clamped to block 0, which every table has) and raises the status word.
// REDUCE: a lane per pair walks the row and writes the dot product.
template <int D4C, bool REDUCE>
__global__ __launch_bounds__(256) void ffm_fwd_kernel(const FfmPack P, const int F, const int D, const long long B,
                                                      float* __restrict__ out, const long long out_stride_b,
                                                      int* __restrict__ status, const int spw, const unsigned n_tasks) {
  __shared__ FfmField sf[RBX_MAX_FIELDS];
  __shared__ unsigned short s_pair[kFfmMaxPairs];
  {
    const int words = F * static_cast<int>(sizeof(FfmField) / 4);
    const int* src = reinterpret_cast<const int*>(&P);
    int* dst = reinterpret_cast<int*>(sf);
    for (int i = threadIdx.x; i < words; i += blockDim.x) dst[i] = src[i];
  }
  const int npairs = F * (F - 1) / 2;
  for (int p = threadIdx.x; p < npairs; p += blockDim.x) {
    int i = 0, rem = p;
    while (rem >= F - 1 - i) {
      rem -= F - 1 - i;
      ++i;
    }
    s_pair[p] = static_cast<unsigned short>((i << 8) | (i + 1 + rem));
  }
  __syncthreads();
  const int D4 = D4C > 0 ? D4C : D / 4;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const unsigned n_waves = gridDim.x * (blockDim.x >> 6);
  for (unsigned task = blockIdx.x * (blockDim.x >> 6) + wid; task < n_tasks; task += n_waves) {
    const long long s0 = static_cast<long long>(task) * spw;
    int x = -1;
    {
      const int sl = lane / F, f = lane - sl * F;
      const long long s = s0 + sl;
      if (sl < spw && s < B) {
        const FfmField& fd = sf[f];
        const long long id = load_id(fd.ids, s * fd.stride_b, fd.dtype);
        if (id >= 0 && id < fd.nblocks) x = static_cast<int>(id);
        else if (status != nullptr) atomicOr(status, 1);
      }
    }
    const int ns = (B - s0 < spw) ? static_cast<int>(B - s0) : spw;
    for (int sl = 0; sl < ns; ++sl) {
      float* __restrict__ orow = out + (s0 + sl) * out_stride_b;
      const int base = sl * F;
      const int units = REDUCE ? npairs : npairs * D4;
      for (int r0 = 0; r0 < units; r0 += 64) {               // (uniform trip count: every lane takes part in the shuffles)
        const int r = r0 + lane;
        const bool live = r < units;
        const int rr = live ? r : 0;
        const int p = REDUCE ? rr : rr / D4;
        const int d4 = REDUCE ? 0 : rr - p * D4;
        const unsigned ij = s_pair[p];
        const int i = static_cast<int>(ij >> 8), j = static_cast<int>(ij & 255u);
        const int xi = __shfl(x, base + i, 64), xj = __shfl(x, base + j, 64);
        const bool ok = xi >= 0 && xj >= 0;
        const float* ra = sf[i].table + (static_cast<size_t>(xi < 0 ? 0 : xi) * F + j) * D + d4 * 4;
        const float* rb = sf[j].table + (static_cast<size_t>(xj < 0 ? 0 : xj) * F + i) * D + d4 * 4;
        if constexpr (REDUCE) {
          float acc = 0.f;
          for (int q = 0; q < D4; ++q) {
            const float4 a = *reinterpret_cast<const float4*>(ra + q * 4);
            const float4 b = *reinterpret_cast<const float4*>(rb + q * 4);
            acc += a.x * b.x;
            acc += a.y * b.y;
            acc += a.z * b.z;
            acc += a.w * b.w;
          }
          if (live) __builtin_nontemporal_store(ok ? acc : 0.f, orow + r);
        } else {
          const float4 a = *reinterpret_cast<const float4*>(ra);
          const float4 b = *reinterpret_cast<const float4*>(rb);
          f32x4 o;
          o.x = ok ? a.x * b.x : 0.f;
          o.y = ok ? a.y * b.y : 0.f;
          o.z = ok ? a.z * b.z : 0.f;
          o.w = ok ? a.w * b.w : 0.f;
          if (live) __builtin_nontemporal_store(o, reinterpret_cast<f32x4*>(orow + static_cast<size_t>(r) * 4));
        }
      }
    }
  }
}

// ---- backward: the reduce's policy ------------------------------------------------------------------------------------
// A sorted pair is (block x of table i, sample b); its contribution is F*D wide: column block j != i holds
// dout[b, p(i,j), :] * table_j[x_j(b)*F + i, :], column block i is zero.  The ids of the other fields are read in place
// through the descriptor array the backward leaves in its workspace (the reduce kernels' argument block has no room for
// it beside their RedPack).  A partner id out of range contributes zeros, as its block read as zeros in the forward.
struct FfmPolicy {
  static constexpr bool kHasCount = false;
  struct Args {
    const FfmField* pack;  // [F], device
    const float* dout;
    long long stride_b;
    int F, D;
    int reduce_sum;
    int accumulate;
  };
  template <int G, int NV>
  static __device__ __forceinline__ void fetch(const Args& a, const RedField& fd, unsigned b, int lane_g,
                                               Frag<G, NV, true>& frag, float& w) {
    w = 1.0f;
    const int i = fd.slot;
    const int F = a.F, D = a.D;
    const int dim = F * D;
    const float* drow = a.dout + static_cast<long long>(b) * a.stride_b;
#pragma unroll
    for (int u = 0; u < NV; ++u) {
      const int e = (lane_g + u * G) * 4;
      const bool in = e < dim;
      const int ec = in ? e : 0;
      const int j0 = ec / D, d = ec - j0 * D;
      const bool off_diag = in && j0 != i;
      const int j = (j0 != i) ? j0 : (i == 0 ? 1 : 0);        // (a field that exists: the addresses below stay valid)
      const int lo = i < j ? i : j, hi = i < j ? j : i;
      const int p = lo * F - lo * (lo + 1) / 2 + (hi - lo - 1);
      const FfmField fj = a.pack[j];
      const long long id = load_id(fj.ids, static_cast<long long>(b) * fj.stride_b, fj.dtype);
      const bool ok = off_diag && id >= 0 && id < fj.nblocks;
      const float* row = fj.table + (static_cast<size_t>(ok ? id : 0) * F + i) * D + d;
      const float4 t = *reinterpret_cast<const float4*>(row);
      float4 g;
      if (a.reduce_sum) {
        const float s = drow[p];
        g = make_float4(s, s, s, s);
      } else {
        g = *reinterpret_cast<const float4*>(drow + static_cast<size_t>(p) * D + d);
      }
      frag.a[u * 4 + 0] = ok ? g.x * t.x : 0.f;
      frag.a[u * 4 + 1] = ok ? g.y * t.y : 0.f;
      frag.a[u * 4 + 2] = ok ? g.z * t.z : 0.f;
      frag.a[u * 4 + 3] = ok ? g.w * t.w : 0.f;
    }
  }
  static __device__ __forceinline__ float weight(const Args&, float w) { return w; }
  template <class Fr>
  static __device__ __forceinline__ void prefetch(const Args& a, const RedField& fd, unsigned row, int lane_g, Fr& pre) {
    if (a.accumulate) pre.add_from(fd.grad + static_cast<size_t>(row) * fd.dim, fd.dim, lane_g);
  }
  template <class Fr>
  static __device__ __forceinline__ void prefetch_raw(const Args& a, const RedField& fd, unsigned row, int lane_g, Fr& pre) {
    if (a.accumulate) pre.load_from(fd.grad + static_cast<size_t>(row) * fd.dim, fd.dim, lane_g);
  }
  template <class Fr>
  static __device__ __forceinline__ void flush(const Args&, const RedField& fd, unsigned row, const Fr& acc, float,
                                               const Fr& pre, int lane_g) {
    Fr o = acc;
    frag_add(o, pre);
    o.store_nt(fd.grad + static_cast<size_t>(row) * fd.dim, fd.dim, lane_g);
  }
};
// a fetch holds the partner row AND the upstream row: two lookups in flight where a lane's share is 16 floats
template <>
struct ReduceWideBatch<FfmPolicy> {
  static constexpr int of(int per_lane) { return per_lane >= 16 ? 2 : 4; }
};
// column block i of a contribution is zero while the others are not: the lanes of a group disagree about "zero"
template <>
struct ReduceLaneZeros<FfmPolicy> {
  static constexpr bool value = true;
};

__global__ __launch_bounds__(64) void ffm_pack_kernel(const FfmPack P, const int F, FfmField* __restrict__ dst) {
  const int words = F * static_cast<int>(sizeof(FfmField) / 4);
  const int* src = reinterpret_cast<const int*>(&P);
  int* d = reinterpret_cast<int*>(dst);
  for (int i = threadIdx.x; i < words; i += blockDim.x) d[i] = src[i];
}

// ---- host ------------------------------------------------------------------------------------------------------------
static size_t ffm_align(size_t v) { return (v + 255) / 256 * 256; }

// every refusal of the header, the kernels' descriptor array, and the [vocab / F, F*D] views the sort and the reduce take
static int ffm_check(const rbx_field_t* fields, int F, int64_t B, FfmPack* pack, rbx_field_t* view, int* dim) {
  if (fields == nullptr) return fail(RBX_ERR_INVALID, "ffm: fields is NULL");
  if (B < 0) return fail(RBX_ERR_INVALID, "ffm: batch=%lld", static_cast<long long>(B));
  if (F < 2 || F > RBX_MAX_FIELDS) return fail(RBX_ERR_UNSUPPORTED, "ffm: n_fields=%d not in [2,%d]", F, RBX_MAX_FIELDS);
  const int D = fields[0].dim;
  if (D <= 0 || D % 4 != 0 || D > 128) return fail(RBX_ERR_UNSUPPORTED, "ffm: dim=%d is not a multiple of 4 in [4,128]", D);
  if (F * D > 1024) return fail(RBX_ERR_UNSUPPORTED, "ffm: F*D=%d exceeds the reduce's lane group (1024 floats)", F * D);
  for (int i = 0; i < F; ++i) {
    const rbx_field_t& f = fields[i];
    if (f.kind != RBX_FIELD_CATEGORICAL || f.pool != RBX_POOL_NONE || f.seq_len != 1)
      return fail(RBX_ERR_UNSUPPORTED, "ffm: field %d is not a one-id categorical feature", i);
    if (f.dim != D) return fail(RBX_ERR_UNSUPPORTED, "ffm: field %d has dim %d, field 0 has %d", i, f.dim, D);
    if (f.ids == nullptr || f.table == nullptr) return fail(RBX_ERR_INVALID, "ffm: field %d: NULL ids / table", i);
    if (f.ids_dtype < RBX_I32 || f.ids_dtype > RBX_F64) return fail(RBX_ERR_INVALID, "ffm: field %d: bad ids_dtype", i);
    if (f.table_stride != 0 && f.table_stride != D)
      return fail(RBX_ERR_UNSUPPORTED, "ffm: field %d: table_stride %lld != dim", i, static_cast<long long>(f.table_stride));
    if (f.padding_idx != RBX_NO_ID) return fail(RBX_ERR_UNSUPPORTED, "ffm: field %d has a padding_idx", i);
    if (f.vocab < F || f.vocab > INT_MAX)
      return fail(RBX_ERR_INVALID, "ffm: field %d: vocab=%lld holds no block of %d rows", i, static_cast<long long>(f.vocab), F);
    if ((reinterpret_cast<uintptr_t>(f.table) & 15) != 0 || (reinterpret_cast<uintptr_t>(f.grad) & 15) != 0)
      return fail(RBX_ERR_UNSUPPORTED, "ffm: field %d: table / grad is not 16-byte aligned", i);
    for (int k = 0; k < i; ++k)
      if (fields[k].table == f.table) return fail(RBX_ERR_UNSUPPORTED, "ffm: fields %d and %d share a table", k, i);
    FfmField& q = pack->f[i];
    q.ids = f.ids;
    q.table = f.table;
    q.stride_b = f.ids_stride_b;
    q.nblocks = static_cast<int>(f.vocab / F);
    q.dtype = f.ids_dtype;
    if (view != nullptr) {
      rbx_field_t& v = view[i];
      v = f;
      v.vocab = f.vocab / F;
      v.dim = F * D;
      v.out_off = 0;
      v.mask_id = RBX_NO_ID;
      v.ids_stride_l = 0;
      v.table_stride = 0;
    }
  }
  *dim = D;
  return RBX_OK;
}

static int ffm_plan(const rbx_field_t* fields, int F, int64_t B, FfmPack* pack, BwdPlan* p, int* dim, size_t* bytes) {
  rbx_field_t view[RBX_MAX_FIELDS];
  int rc = ffm_check(fields, F, B, pack, view, dim);
  if (rc != RBX_OK) return rc;
  rc = make_plan(view, F, B, nullptr, 0, p);
  if (rc != RBX_OK) return rc;
  if (!p->vec) return fail(RBX_ERR_UNSUPPORTED, "ffm: the gradients are not float4-addressable");
  *bytes = ffm_align(p->bytes) + sizeof(FfmPack);
  return RBX_OK;
}

template <bool REDUCE>
static void ffm_launch_fwd(const FfmPack& pack, int F, int D, int64_t B, float* out, int64_t stride, int* status,
                           hipStream_t s) {
  const int spw = 64 / F;
  const unsigned n_tasks = static_cast<unsigned>((B + spw - 1) / spw);
  unsigned blocks = (n_tasks + 3) / 4;
  if (blocks > static_cast<unsigned>(kCUs * 8)) blocks = kCUs * 8;
#define RBX_FFM_FWD(D4C)                                                                                              \
  hipLaunchKernelGGL((ffm_fwd_kernel<D4C, REDUCE>), dim3(blocks), dim3(256), 0, s, pack, F, D, static_cast<long long>(B), \
                     out, static_cast<long long>(stride), status, spw, n_tasks)
  switch (D / 4) {
    case 1: RBX_FFM_FWD(1); break;
    case 2: RBX_FFM_FWD(2); break;
    case 4: RBX_FFM_FWD(4); break;
    case 8: RBX_FFM_FWD(8); break;
    default: RBX_FFM_FWD(0); break;
  }
#undef RBX_FFM_FWD
}

}  // namespace rbx

extern "C" int rbx_ffm_fwd(const rbx_field_t* fields, int32_t n_fields, int64_t batch, int32_t reduce_sum, float* d_out,
                           int64_t out_stride_b, int32_t* d_status, void* stream) {
  using namespace rbx;
  FfmPack pack;
  int D = 0;
  int rc = ffm_check(fields, n_fields, batch, &pack, nullptr, &D);
  if (rc != RBX_OK) return rc;
  if (batch == 0) return RBX_OK;
  if (d_out == nullptr) return fail(RBX_ERR_INVALID, "ffm_fwd: d_out is NULL");
  const int64_t P = static_cast<int64_t>(n_fields) * (n_fields - 1) / 2;
  if (out_stride_b < (reduce_sum ? P : P * D)) return fail(RBX_ERR_INVALID, "ffm_fwd: out_stride_b below the row width");
  if (batch / (64 / n_fields) >= (1ll << 31)) return fail(RBX_ERR_UNSUPPORTED, "ffm_fwd: batch too large");
  if (!reduce_sum && ((reinterpret_cast<uintptr_t>(d_out) & 15) != 0 || out_stride_b % 4 != 0))
    return fail(RBX_ERR_UNSUPPORTED, "ffm_fwd: d_out must be 16-byte aligned with a row stride that is a multiple of 4");
  if (reduce_sum && (reinterpret_cast<uintptr_t>(d_out) & 3) != 0) return fail(RBX_ERR_UNSUPPORTED, "ffm_fwd: misaligned d_out");
  if (reduce_sum) ffm_launch_fwd<true>(pack, n_fields, D, batch, d_out, out_stride_b, d_status, as_stream(stream));
  else ffm_launch_fwd<false>(pack, n_fields, D, batch, d_out, out_stride_b, d_status, as_stream(stream));
  return check_launch("ffm_fwd_kernel");
}

extern "C" size_t rbx_ffm_bwd_workspace_size(const rbx_field_t* fields, int32_t n_fields, int64_t batch) {
  using namespace rbx;
  FfmPack pack;
  BwdPlan p;
  int D = 0;
  size_t bytes = 0;
  if (ffm_plan(fields, n_fields, batch, &pack, &p, &D, &bytes) != RBX_OK) return 0;
  return bytes;
}

extern "C" int rbx_ffm_sort(const rbx_field_t* fields, int32_t n_fields, int64_t batch, void* d_workspace,
                            size_t workspace_bytes, int32_t* d_status, void* stream) {
  using namespace rbx;
  FfmPack pack;
  BwdPlan p;
  int D = 0;
  size_t bytes = 0;
  int rc = ffm_plan(fields, n_fields, batch, &pack, &p, &D, &bytes);
  if (rc != RBX_OK) return rc;
  if (batch == 0 || p.n_lookups == 0) return RBX_OK;
  if (d_workspace == nullptr || workspace_bytes < bytes)
    return fail(RBX_ERR_WORKSPACE, "ffm_sort: workspace %zu B < required %zu B", workspace_bytes, bytes);
  return run_sort(p, static_cast<char*>(d_workspace), d_status, as_stream(stream));
}

extern "C" int rbx_ffm_bwd(const rbx_field_t* fields, int32_t n_fields, int64_t batch, int32_t reduce_sum,
                           const float* d_dout, int64_t dout_stride_b, int32_t accumulate, void* d_workspace,
                           size_t workspace_bytes, void* stream) {
  using namespace rbx;
  FfmPack pack;
  BwdPlan p;
  int D = 0;
  size_t bytes = 0;
  int rc = ffm_plan(fields, n_fields, batch, &pack, &p, &D, &bytes);
  if (rc != RBX_OK) return rc;
  if (batch == 0 || p.n_lookups == 0) return RBX_OK;
  if (d_dout == nullptr) return fail(RBX_ERR_INVALID, "ffm_bwd: d_dout is NULL");
  const int64_t P = static_cast<int64_t>(n_fields) * (n_fields - 1) / 2;
  if (dout_stride_b < (reduce_sum ? P : P * D)) return fail(RBX_ERR_INVALID, "ffm_bwd: dout_stride_b below the row width");
  if (!reduce_sum && ((reinterpret_cast<uintptr_t>(d_dout) & 15) != 0 || dout_stride_b % 4 != 0))
    return fail(RBX_ERR_UNSUPPORTED, "ffm_bwd: d_dout must be 16-byte aligned with a row stride that is a multiple of 4");
  if (reduce_sum && (reinterpret_cast<uintptr_t>(d_dout) & 3) != 0) return fail(RBX_ERR_UNSUPPORTED, "ffm_bwd: misaligned d_dout");
  if (d_workspace == nullptr || workspace_bytes < bytes)
    return fail(RBX_ERR_WORKSPACE, "ffm_bwd: workspace %zu B < required %zu B", workspace_bytes, bytes);
  char* ws = static_cast<char*>(d_workspace);
  hipStream_t s = as_stream(stream);
  FfmField* d_pack = reinterpret_cast<FfmField*>(ws + ffm_align(p.bytes));
  hipLaunchKernelGGL(ffm_pack_kernel, dim3(1), dim3(64), 0, s, pack, n_fields, d_pack);
  rc = check_launch("ffm_pack_kernel");
  if (rc != RBX_OK) return rc;
  const int cur = p.passes & 1;
  const unsigned* keys = reinterpret_cast<const unsigned*>(ws + p.off_keys[cur]);
  const unsigned* vals = reinterpret_cast<const unsigned*>(ws + p.off_vals[cur]);
  const FfmPolicy::Args args = {d_pack, d_dout, static_cast<long long>(dout_stride_b), n_fields, D, reduce_sum ? 1 : 0,
                                accumulate ? 1 : 0};
  return dispatch_reduce<FfmPolicy, true>(p, args, keys, vals, ws, s);
}
