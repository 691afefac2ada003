/* recbox_hip.h -- C ABI of librecbox_hip.so (gfx950 / MI355X only).
 *
 * Drop-in boundary for the embedding-lookup + feature-interaction hot path of
 * reczoo/RecBox.  The reference has no FFI of its own (it is pure Python on
 * PyTorch): each entry point below replaces the ATen op
 * sequence that one reference nn.Module dispatches, and cites that module
 * (paths relative to /root/reference/recbox).  INTEGRATION.md shows the ctypes
 * stub a maintainer would add to call these from the reference's own layers.
 *
 * Conventions
 *   - plain C: pointers and sizes only, no C++ or torch types;
 *   - every pointer named d_* / inside rbx_field_t is a DEVICE pointer, every
 *     other pointer is a HOST pointer;
 *   - the caller owns all memory including workspaces (query *_workspace_size);
 *     the library allocates nothing persistent and keeps no global state but a
 *     thread-local error string;
 *   - kernels are enqueued on `stream` (a hipStream_t passed as void*; NULL is
 *     the default stream) and never synchronise; calls are re-entrant across
 *     streams;
 *   - return value: 0 on success, a negative rbx_status_t otherwise, message in
 *     rbx_last_error();
 *   - all floating point is IEEE fp32; ids are exact (bit-identical row choice).
 */
#ifndef RECBOX_HIP_H
#define RECBOX_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RBX_VERSION 124          /* 0.1.24: rbx_sort_chained (the id sort in 1 + passes launches), then rbx_bag_t / rbx_embed_csr_fwd / _bwd_workspace_size / _sort / _bwd (ragged bags; additions only, the number stays); 0.1.23: rbx_fm_tier_c / rbx_fm_rezero_fusable, rbx_linear_fwd_bnstats / rbx_linear_dx_bnsums / rbx_batchnorm_*_from_partials removed (variants that lost their A/B); 0.1.22: rbx_cin_outer_*; 0.1.21: rbx_prelu_* / rbx_dropout / rbx_dice_* (csrc/rbx_act.hip); 0.1.20: rbx_fm_quad (rbx_fm_fwd's kernel for ids that are columns of one batch tensor); 0.1.19: rbx_seqblock_* (the row-local chains of a SASRec block as single passes); 0.1.18: rbx_fm_tier_c (the fused FM backward's sort-free tier C), rbx_opt_advance, rbx_opt_t.d_step_size, rbx_comm_bind_collectives takes ncclCommUserRank; 0.1.17: rbx_all_reduce / rbx_all_gather / rbx_comm_bind_collectives (every collective of the sharded step on the caller's stream); 0.1.16: rbx_linear_dx_scaled / rbx_linear_dwdb_scaled, rbx_rowscale_seq / rbx_seq_colsum; 0.1.15: rbx_linear_fwd_bnstats / rbx_linear_dx_bnsums / rbx_batchnorm_*_from_partials; 0.1.14: rbx_split_bf16 / _register / _unregister (f32 GEMM on the bf16 matrix cores); 0.1.13: rbx_fm_sort_phases, rbx_fm_bwd phases bits 3 / 4 (round 3: the fused FM backward in
                                  * two tiers); 0.1.11: rbx_fm_fwd grew d_prob; 0.1.10: rbx_field_t grew table_stride (round 2) */
#define RBX_MAX_FIELDS 64        /* fields per call */
#define RBX_NO_ID INT64_MIN      /* "no such id" for padding_idx / mask_id */

typedef enum {
  RBX_OK = 0,
  RBX_ERR_INVALID = -1,          /* bad argument (ValueError on the Python side) */
  RBX_ERR_LAUNCH = -2,           /* HIP launch / runtime failure (RuntimeError) */
  RBX_ERR_WORKSPACE = -3,        /* workspace too small */
  RBX_ERR_UNSUPPORTED = -4       /* NotImplementedError on the Python side */
} rbx_status_t;

/* dtype of an id / value column as it reaches the layer (int64,
 * int32, or float64 when the ranking loader hstacks the split; the kernels do
 * the reference's `.long()` / `.float()` casts in registers). */
typedef enum { RBX_I32 = 0, RBX_I64 = 1, RBX_F32 = 2, RBX_F64 = 3 } rbx_dtype_t;

typedef enum {
  RBX_FIELD_CATEGORICAL = 0,     /* nn.Embedding(vocab, dim)(ids.long()) */
  RBX_FIELD_NUMERIC = 1,         /* nn.Linear(1, dim, bias=False)(x.float().view(-1,1)) */
  RBX_FIELD_DENSE = 2            /* rechub DenseFeature: x.float() copied, dim == 1 */
} rbx_field_kind_t;

typedef enum {
  RBX_POOL_NONE = 0,             /* one id per sample */
  RBX_POOL_SUM = 1,              /* recbox MaskedSumPooling: plain sum over L */
  RBX_POOL_MEAN_VALUE = 2,       /* recbox MaskedAveragePooling: sum / (#rows with sum_d != 0 + eps) */
  RBX_POOL_MEAN_ID = 3,          /* rechub AveragePooling: sum_{id != mask_id} / (count + eps) */
  RBX_POOL_SUM_ID = 4,           /* rechub SumPooling with InputMask */
  RBX_POOL_CONCAT = 5,           /* rechub ConcatPooling: keep [L, dim] */
  RBX_POOL_MAX = 6               /* ragged bags only (rbx_embed_csr_fwd_max): elementwise max, torch's EmbeddingBag mode="max";
                                  * honours mask_id when one is set, ignores eps; the padded lookup refuses it */
} rbx_pool_t;

/* One feature of a multi-table lookup.  Output slot of sample b:
 *   d_out + b * out_stride_b + out_off   (dim floats; L*dim for POOL_CONCAT). */
typedef struct rbx_field {
  const void*  ids;              /* [B] or [B, seq_len] ids; numeric/dense: values */
  const float* table;            /* [vocab, dim] table; numeric: Linear weight as [dim]; dense: NULL */
  float*       grad;             /* backward only: dense grad, same shape as table (accumulated into) */
  int64_t      ids_stride_b;     /* element stride between samples */
  int64_t      ids_stride_l;     /* element stride inside a sequence */
  int64_t      vocab;
  int64_t      padding_idx;      /* nn.Embedding.padding_idx: row gets zero grad; RBX_NO_ID if unset */
  int64_t      mask_id;          /* *_ID pools: lookups equal to it get weight 0; RBX_NO_ID if unset */
  int64_t      out_off;          /* float offset of the slot inside an output row */
  int32_t      dim;
  int32_t      seq_len;          /* 1 unless a sequence feature */
  int32_t      ids_dtype;        /* rbx_dtype_t */
  int32_t      kind;             /* rbx_field_kind_t */
  int32_t      pool;             /* rbx_pool_t */
  float        eps;              /* MEAN pools: 1e-12 (recbox), 1e-16 (rechub), 1e-8 (RecBole) */
  int64_t      table_stride;     /* floats between consecutive table rows; 0 = dim (a contiguous [vocab, dim] table).
                                  * Only rbx_fm_fwd / rbx_fm_sort / rbx_fm_bwd / rbx_fm_rezero honour other values: the
                                  * embedding row and the dim-1 LR weight of an id may then share ONE padded row of a
                                  * packed [vocab, stride] storage (emb.table = base, lr.table = base + D, both with
                                  * table_stride = stride: one 128-byte line per lookup instead of two); every other
                                  * entry point rejects a stride != dim.  Gradients stay contiguous [vocab, dim]. */
} rbx_field_t;

const char* rbx_last_error(void);
int rbx_version(void);

/* ---- K1/K2: multi-table gather (+ fused sequence pooling) ------------------
 * Replaces, in ONE launch over all fields, the per-feature Python loop of
 *   core/pytorch/layers/embedding.py:116-138  (EmbeddingDictLayer.forward + callbacks),
 *   ranking/pytorch/layers/embeddings/feature_embedding.py:188-214 (+ dict2tensor :169-186),
 *   third_party/rechub/basic/layers.py:66-116 (EmbeddingLayer.forward, InputMask, pooling :176-230),
 * i.e. nn.Embedding / nn.Linear(1,D) / masked mean|sum pooling / stack|cat.
 * d_row_scale: [F, B] floats, written for MEAN pools (1/(count+eps)), read by the
 * backward; may be NULL when no MEAN pool is present.
 * d_status: optional int32 flag word, set non-zero when an id is out of range
 * (the reference raises IndexError); out-of-range lookups read as zero rows. */
int rbx_embed_fwd(const rbx_field_t* fields, int32_t n_fields, int64_t batch,
                  float* d_out, int64_t out_stride_b, float* d_row_scale,
                  int32_t* d_status, void* stream);

/* ---- K3: embedding backward = sorted, segmented, deterministic scatter-add ---
 * Replaces autograd's embedding_dense_backward (+ pooling / stack backward) of the
 * modules above.  Two phases so that the id sort can run early (ids are known in
 * the forward) on another stream:
 *   rbx_embed_sort   : builds (global row, lookup) pairs for every categorical
 *                      lookup, drops padding_idx / masked ids, radix-sorts them.
 *   rbx_embed_bwd    : segment-reduces d_out rows in sorted order and adds each
 *                      touched row ONCE into fields[f].grad (dense [vocab,dim]).
 *                      accumulate == 0: the caller pre-zeroed the grads, touched rows
 *                      are stored (no read); accumulate != 0: read-modify-write into
 *                      existing grads.  Numeric fields get
 *                      grad[d] += sum_b x_b * d_out[b, off+d].  Features that
 *                      share a table (same `table` pointer) are merged.
 * Results are run-to-run deterministic (no float atomics). */
size_t rbx_embed_bwd_workspace_size(const rbx_field_t* fields, int32_t n_fields, int64_t batch);
int rbx_embed_sort(const rbx_field_t* fields, int32_t n_fields, int64_t batch,
                   void* d_workspace, size_t workspace_bytes, int32_t* d_status, void* stream);
int rbx_embed_bwd(const rbx_field_t* fields, int32_t n_fields, int64_t batch,
                  const float* d_dout, int64_t out_stride_b, const float* d_row_scale,
                  int32_t accumulate, void* d_workspace, size_t workspace_bytes, void* stream);
/* Same, with one indirection: sample b reads its upstream gradient from row d_dout_index[b] of d_dout (int32, [batch])
 * instead of row b.  The owner side of the sharded exchange (rbx_shard_serve below) uses it: many received lookups
 * share one gradient row (the pooled history of a sample), which is then never expanded in memory. */
int rbx_embed_bwd_indexed(const rbx_field_t* fields, int32_t n_fields, int64_t batch,
                          const float* d_dout, int64_t out_stride_b, const int32_t* d_dout_index,
                          const float* d_row_scale, int32_t accumulate, void* d_workspace, size_t workspace_bytes,
                          void* stream);

/* ---- K1-K3 for RAGGED bags (CSR): indices / offsets gather-pool, forward and backward (csrc/rbx_embed_csr.hip) ----
 * The same pooled lookups as a sequence feature of rbx_embed_fwd, for a caller that holds its multi-hot ids unpadded: the
 * layout of torch.nn.EmbeddingBag and of every loader that does not pad to max_len.  Semantics kept: the pooling variants
 * of core/pytorch/layers/sequence.py:4-20 (MaskedSumPooling / MaskedAveragePooling) and of
 * third_party/rechub/basic/layers.py:176-230 (InputMask + SumPooling / AveragePooling), each exactly as rbx_pool_t
 * defines it for padded ids -- a bag is the history without its padded tail.
 *   indices  flat [nnz] ids of any rbx_dtype_t (the `.long()` cast happens in registers), element stride indices_stride;
 *   offsets  [batch + 1], RBX_I32 or RBX_I64, contiguous: bag b = indices[offsets[b] : offsets[b + 1]).  offsets[0] may be
 *            > 0 and offsets[batch] < nnz (ids outside every bag are never looked up); a bag may be empty: a zero output
 *            row, and for the mean pools a scale of 1 / (0 + eps) times a zero sum = 0.
 *   pool     RBX_POOL_SUM, RBX_POOL_SUM_ID, RBX_POOL_MEAN_ID or RBX_POOL_MEAN_VALUE, or RBX_POOL_MAX through the calls of its
 *            own below; RBX_POOL_NONE / RBX_POOL_CONCAT return RBX_ERR_UNSUPPORTED.
 * Malformed offsets cannot make a kernel read outside indices[0, nnz): every bag is clamped to 0 <= begin <= end <= nnz
 * before an index is read, and bit 1 (value 2) of *d_status is set when the clamp changed anything (a decreasing pair, a
 * negative value, a value above nnz).  Ids outside [0, vocab) set bit 0 and read as zero rows, as in rbx_embed_fwd.
 *   rbx_embed_csr_fwd   one launch per (float4 | scalar) class over all bags of the call; bag b of descriptor i goes to
 *                       d_out + b * out_stride_b + bags[i].out_off -- the slots may sit inside the [batch, width] block
 *                       an rbx_embed_fwd call fills.  d_row_scale [n_bags, batch]: written for the mean pools (may be
 *                       NULL without one).  A bag is summed in list order by the lane-group form rbx_embed_fwd uses for
 *                       that dim: bit-equal to the padded call over the same live ids.
 *   rbx_embed_csr_sort  (global row, bag) pairs of the in-range, unmasked, non-padding ids that lie inside a bag, plus an
 *                       int32 lookup -> bag map in the workspace; ONE segmented radix sort per call (the passes of
 *                       rbx_embed_sort; key width derived the same way: the bits of the largest table group's row count).
 *   rbx_embed_csr_bwd   the contract of rbx_embed_bwd: dense [vocab, dim] gradients into bags[i].grad (NULL = frozen),
 *                       every touched row written once, the padding_idx row zero, masked ids contribute nothing, bags
 *                       that share a `table` pointer are merged, accumulate as there, no float atomics: bit-identical
 *                       from run to run.  The mean scale is read per bag (d_row_scale[i * batch + b]).
 * Limits: n_bags <= RBX_MAX_BAGS; nnz of one descriptor and batch at most 2^26; the nnz of a call together below 2^31
 * (positions outside every bag take part in the sort as dropped pairs); dims as rbx_embed_fwd (1..256 lane-group units).
 *
 * Per-sample weights (torch's per_sample_weights; RBX_POOL_SUM and RBX_POOL_SUM_ID only).  rbx_bag_t is unchanged: the
 * weights travel as a host array of n_bags device pointers, entry i an fp32 [bags[i].nnz] contiguous array whose element
 * j belongs to indices[j], or NULL = descriptor i is unweighted (a call may mix both; d_weights itself may be NULL).
 *   out[b, slot]  = sum over the usable j of bag b of  w[j] * table[id_j]
 *   dTable[id_j] += w[j] * dY[b, slot]                (the padding_idx row stays zero)
 *   dw[j]         = < dY[b, slot], table[id_j] >      for usable j inside a bag, 0 for every other position
 * "usable" as above: inside a clamped bag, id in [0, vocab), not the mask_id of RBX_POOL_SUM_ID.  The padding_idx id is
 * read and weighted in the forward like any row and gets the dw of that read; only its table-gradient row is zero.  A
 * non-NULL weight array (or weight gradient) on a mean-pool descriptor returns RBX_ERR_UNSUPPORTED with nothing launched.
 * No weight is read outside w[0, nnz): weights are read at the positions ids are read at.  No float atomics; with every
 * weight exactly 1.0f outputs and table gradients are bit-equal to the unweighted calls on the same bags.
 *   rbx_embed_csr_fwd_weighted   rbx_embed_csr_fwd with the factor; unweighted descriptors run as they do there (a mean
 *                                pool among them is computed, but its row scale is not kept: no d_row_scale here).
 *   rbx_embed_csr_sort_weighted  rbx_embed_csr_sort with pairs whose value is the lookup's position inside its index
 *                                array instead of the bag; same workspace size (rbx_embed_csr_bwd_workspace_size).  The
 *                                workspace it leaves is for rbx_embed_csr_bwd_weighted only, and that call takes no other.
 *   rbx_embed_csr_bwd_weighted   rbx_embed_csr_bwd over that sort: bag = map[position], factor = w[position].  Mean-pool
 *                                descriptors with a gradient are refused by both (RBX_ERR_UNSUPPORTED): their backward
 *                                needs the row scale of the unweighted path.
 *   rbx_embed_csr_weight_grad    d_dweights: host array of n_bags device pointers, entry i an fp32 [nnz] array or NULL (no
 *                                gradient wanted).  Every element of a non-NULL array is defined after the call (cleared
 *                                by a memset node, then the usable positions are written).  Needs no sort.
 *
 * Training a large table (persistent gradients, sparse-row optimiser step).  After rbx_embed_csr_sort[_weighted] +
 * rbx_embed_csr_bwd[_weighted] the workspace still holds the sorted pairs: the head of each run of equal keys names one
 * touched row.  Both calls below read keys and plan slots only, so they take the workspace of either sort; descriptor
 * rules and refusals are those of the calls above, made before anything is launched; a workspace smaller than
 * rbx_embed_csr_bwd_workspace_size returns RBX_ERR_WORKSPACE; batch == 0 or no lookups: RBX_OK, nothing launched.
 *   rbx_embed_csr_rezero         the contract of rbx_embed_rezero: zeros to exactly the rows of bags[i].grad that the
 *                                previous rbx_embed_csr_bwd[_weighted] on this workspace stored (bags[i].nnz as in that
 *                                call: it fixes the workspace layout).  Only for tables that get their gradient from that
 *                                call alone.
 *   rbx_embed_csr_sparse_update  the contract of rbx_embed_sparse_update (rules and rbx_opt_t below): one SGD / Adagrad /
 *                                lazy-Adam step on exactly the touched rows of bags[i].table and of d_state1[i] /
 *                                d_state2[i] -- indexed by DESCRIPTOR i (entries of frozen descriptors are not looked at;
 *                                descriptors that share a table pass the same pointers and the row is stepped once).
 *                                Untouched rows, padding_idx rows, mask_id ids of the _ID pools, ids outside [0, vocab)
 *                                and positions outside every bag are neither read nor written.  A rule without its state
 *                                array returns RBX_ERR_INVALID.  clear_grad != 0: the lane group that steps a row writes
 *                                zeros over that gradient row once it holds it in registers (non-temporal stores): the
 *                                step and the re-zero in one launch, table and state bit-equal to clear_grad = 0.
 *
 * Max pool (RBX_POOL_MAX; torch.nn.EmbeddingBag(mode="max"), whose CPU result is the reference).  "usable" as above, with
 * mask_id honoured whenever it is set (torch excludes padding_idx from the max: pass it as mask_id).
 *   out[b, out_off + d]    = max over the usable j of bag b of table[id_j][d]; a bag without a usable id (empty, all masked,
 *                            all out of range) gives a row of zeros, never -inf, and no table gradient
 *   argpos[b, out_off + d] = the position j in [0, nnz) of the winner in the descriptor's index array, -1 where the bag
 *                            had no usable id.  Ties: the LOWEST position wins (torch: strict >, first occurrence)
 *   dTable[id_argpos[b, c]][d] += dY[b, c], summed through the sorted pairs: no float atomics, the same bits from run to
 *                            run; the padding_idx row is read in the forward and keeps a zero gradient row
 * Table values are finite: NaN and +-inf in a table are outside the contract.  Status bits and the offset clamp as above.
 *   rbx_embed_csr_fwd_max  every descriptor must be RBX_POOL_MAX (else RBX_ERR_UNSUPPORTED).  d_argpos: int32 [batch,
 *                          arg_stride_b], a descriptor's columns at out_off .. out_off + dim as in d_out.  long_threshold as in
 *                          the `_long` calls below; 0 = no hand-off and no workspace.  A max selects and never rounds, so the
 *                          long form is BIT-EQUAL to the lane-group walk at every threshold, d_out and d_argpos alike.
 *   rbx_embed_csr_fwd_max_workspace_size  rbx_embed_csr_fwd_long_workspace_size plus one int32 partial argpos row per
 *                          segment slot; the same guarantees (no pointer read, never shrinks when an nnz grows).
 *   rbx_embed_csr_bwd_max  over the workspace rbx_embed_csr_sort_weighted leaves (position-valued pairs); every descriptor
 *                          RBX_POOL_MAX.  d_argpos is only compared with positions, never used as an address: no content
 *                          of it makes a kernel read out of bounds.  accumulate as rbx_embed_csr_bwd.
 * The calls that never pool -- rbx_embed_csr_bwd_workspace_size, _sort, _sort_weighted, _rezero, _sparse_update -- take
 * RBX_POOL_MAX descriptors like any other; every call that pools a sum or a mean, or takes weights (rbx_embed_csr_fwd,
 * _fwd_long, _fwd_weighted, _fwd_weighted_long, _bwd, _bwd_weighted, _weight_grad, _weight_grad_long), returns
 * RBX_ERR_UNSUPPORTED for one before anything is cleared or launched. */
#define RBX_MAX_BAGS 32
typedef struct rbx_bag {
  const void*  indices;          /* [nnz] ids */
  const void*  offsets;          /* [batch + 1] bag boundaries */
  const float* table;            /* [vocab, dim] */
  float*       grad;             /* backward only: dense grad, same shape as table; NULL = frozen */
  int64_t      nnz;
  int64_t      indices_stride;   /* element stride of indices */
  int64_t      vocab;
  int64_t      padding_idx;      /* row that gets zero grad; RBX_NO_ID if unset */
  int64_t      mask_id;          /* *_ID pools: ids equal to it get weight 0; RBX_NO_ID if unset */
  int64_t      out_off;          /* float offset of the slot inside an output row */
  int32_t      dim;
  int32_t      indices_dtype;    /* rbx_dtype_t */
  int32_t      offsets_dtype;    /* RBX_I32 or RBX_I64 */
  int32_t      pool;             /* rbx_pool_t */
  float        eps;              /* MEAN pools */
  int32_t      reserved;         /* 0 */
} rbx_bag_t;
int rbx_embed_csr_fwd(const rbx_bag_t* bags, int32_t n_bags, int64_t batch, float* d_out, int64_t out_stride_b,
                      float* d_row_scale, int32_t* d_status, void* stream);
size_t rbx_embed_csr_bwd_workspace_size(const rbx_bag_t* bags, int32_t n_bags, int64_t batch);
int rbx_embed_csr_sort(const rbx_bag_t* bags, int32_t n_bags, int64_t batch, void* d_workspace, size_t workspace_bytes,
                       int32_t* d_status, void* stream);
int rbx_embed_csr_bwd(const rbx_bag_t* bags, int32_t n_bags, int64_t batch, const float* d_dout, int64_t out_stride_b,
                      const float* d_row_scale, int32_t accumulate, void* d_workspace, size_t workspace_bytes,
                      void* stream);
int rbx_embed_csr_fwd_weighted(const rbx_bag_t* bags, int32_t n_bags, int64_t batch, const float* const* d_weights,
                               float* d_out, int64_t out_stride_b, int32_t* d_status, void* stream);
int rbx_embed_csr_sort_weighted(const rbx_bag_t* bags, int32_t n_bags, int64_t batch, void* d_workspace,
                                size_t workspace_bytes, int32_t* d_status, void* stream);
int rbx_embed_csr_bwd_weighted(const rbx_bag_t* bags, int32_t n_bags, int64_t batch, const float* const* d_weights,
                               const float* d_dout, int64_t out_stride_b, int32_t accumulate, void* d_workspace,
                               size_t workspace_bytes, void* stream);
int rbx_embed_csr_weight_grad(const rbx_bag_t* bags, int32_t n_bags, int64_t batch, const float* d_dout,
                              int64_t out_stride_b, float* const* d_dweights, int32_t* d_status, void* stream);
int rbx_embed_csr_rezero(const rbx_bag_t* bags, int32_t n_bags, int64_t batch, void* d_workspace, size_t workspace_bytes,
                         void* stream);
struct rbx_opt;                  /* rbx_opt_t, declared with rbx_embed_sparse_update below */
int rbx_embed_csr_sparse_update(const rbx_bag_t* bags, int32_t n_bags, int64_t batch, const void* d_workspace,
                                size_t workspace_bytes, const struct rbx_opt* opt, float* const* d_state1,
                                float* const* d_state2, int32_t clear_grad, void* stream);
size_t rbx_embed_csr_fwd_max_workspace_size(const rbx_bag_t* bags, int32_t n_bags, int64_t batch, int64_t long_threshold);
int rbx_embed_csr_fwd_max(const rbx_bag_t* bags, int32_t n_bags, int64_t batch, int64_t long_threshold, float* d_out,
                          int64_t out_stride_b, int32_t* d_argpos, int64_t arg_stride_b, void* d_workspace,
                          size_t workspace_bytes, int32_t* d_status, void* stream);
int rbx_embed_csr_bwd_max(const rbx_bag_t* bags, int32_t n_bags, int64_t batch, const float* d_dout, int64_t out_stride_b,
                          const int32_t* d_argpos, int64_t arg_stride_b, int32_t accumulate, void* d_workspace,
                          size_t workspace_bytes, void* stream);

/* The long-bag form of the three bag-walking calls above.  They map one lane group to one bag whatever its length, so a
 * few bags of thousands of ids keep a wave (and the launch) waiting for one group.  The `_long` calls take a
 * long_threshold T: a bag of at least T ids (after the clamp) is cut into segments of RBX_CSR_SEGMENT consecutive ids, a
 * wave per segment over the whole grid, and the segments' partial sums are added in ascending segment order.
 *   - a bag shorter than T is summed by its lane group exactly as in the calls above: the same bits;
 *   - a bag of T ids or more has its own, fixed summation order: bit-identical from run to run, NOT bit-equal to the
 *     padded call -- it meets the float64 bound of the sum instead.  With every weight 1.0f the weighted long call is
 *     bit-equal to the unweighted long call;
 *   - long_threshold 0 = never: the calls above, bit for bit (the workspace is then the 256-byte header only).
 * The long bags are found on the device (no host read of offsets: the calls stay capturable in a hipGraph).
 * d_workspace: rbx_embed_csr_fwd_long_workspace_size bytes for the same bags / batch / threshold -- one size serves the
 * three calls; it depends on nnz, dim, batch and the threshold only (no pointer of the descriptors is read), is at least
 * the header for nnz == 0 and never shrinks when an nnz grows.  A smaller workspace returns RBX_ERR_WORKSPACE.  The
 * call clears the header itself (a memset node).  Afterwards the header's int32 word RBX_CSR_WS_SEGMENTS holds the number
 * of segments and word RBX_CSR_WS_LONG_BAGS the number of bags that took the long form -- tests and profiles read them.
 * Well-formed offsets cannot exceed the workspace (the bag lengths of a descriptor sum to at most nnz).  Malformed ones
 * (overlapping bags) can: a bag that finds the list or the partial area full is walked by its lane group in the same
 * launch, as in the calls above; the two words may then read beyond what was used, and every kernel clamps them.  No
 * input makes a kernel read outside indices[0, nnz) or write outside the workspace and d_out; status bits as above.
 * Refusals (pools, dims, NULLs) are those of the calls above and are made before anything is launched. */
#define RBX_CSR_SEGMENT 256      /* ids per segment: a multiple of every lane-group chunk (64, 128, 256) */
#define RBX_CSR_WS_SEGMENTS 0    /* int32 word index into the workspace header */
#define RBX_CSR_WS_LONG_BAGS 1
size_t rbx_embed_csr_fwd_long_workspace_size(const rbx_bag_t* bags, int32_t n_bags, int64_t batch, int64_t long_threshold);
int rbx_embed_csr_fwd_long(const rbx_bag_t* bags, int32_t n_bags, int64_t batch, int64_t long_threshold, float* d_out,
                           int64_t out_stride_b, float* d_row_scale, void* d_workspace, size_t workspace_bytes,
                           int32_t* d_status, void* stream);
int rbx_embed_csr_fwd_weighted_long(const rbx_bag_t* bags, int32_t n_bags, int64_t batch, int64_t long_threshold,
                                    const float* const* d_weights, float* d_out, int64_t out_stride_b, void* d_workspace,
                                    size_t workspace_bytes, int32_t* d_status, void* stream);
int rbx_embed_csr_weight_grad_long(const rbx_bag_t* bags, int32_t n_bags, int64_t batch, int64_t long_threshold,
                                   const float* d_dout, int64_t out_stride_b, float* const* d_dweights, void* d_workspace,
                                   size_t workspace_bytes, int32_t* d_status, void* stream);

/* ---- K4: InnerProductInteraction / rechub FM on a materialised [B,F,D] tensor ---
 * ranking/pytorch/layers/interactions/inner_product.py:40-56,
 * third_party/rechub/basic/layers.py:286-292.
 * mode 0: product_sum -> [B,1]; 1: bi_interaction -> [B,D];
 * mode 2: inner_product -> [B,F(F-1)/2]; 3: elementwise_product -> [B,F(F-1)/2,D].
 * emb_stride_b / demb_stride_b: floats between consecutive samples (>= F*D): the [F, D] block of a sample may
 * be the leading columns of a wider activation row (the flattened embedding layout of rechub's DeepFM). */
int rbx_interaction_fwd(const float* d_emb, int64_t emb_stride_b, int64_t batch, int32_t n_fields, int32_t dim,
                        int32_t mode, float* d_out, void* stream);
int rbx_interaction_bwd(const float* d_emb, int64_t emb_stride_b, const float* d_dout, int64_t batch, int32_t n_fields,
                        int32_t dim, int32_t mode, float* d_demb, int64_t demb_stride_b, void* stream);

/* ---- the pairing step of BilinearInteraction / BilinearInteractionV2
 * (ranking/pytorch/layers/interactions/bilinear_interaction.py:24-90).  out[b, p(i,j), :] = left * right[b, j, :] over
 * the F(F-1)/2 pairs i < j in triu order; per_pair == 0: left[B, F, D] = hidden (e_i W or e_i W_i: field_all /
 * field_each), indexed by i; per_pair == 1: left[B, P, D] = e_i W_p (field_interaction), indexed by the pair.  The
 * products with W run on rbx_linear_fwd.  Backward writes d_dleft (same shape as left) and d_dright[B, F, D]. */
int rbx_pairmul_fwd(const float* d_left, const float* d_right, int64_t batch, int32_t n_fields, int32_t dim,
                    int32_t per_pair, float* d_out, void* stream);
int rbx_pairmul_bwd(const float* d_left, const float* d_right, const float* d_dout, int64_t batch, int32_t n_fields,
                    int32_t dim, int32_t per_pair, float* d_dleft, float* d_dright, void* stream);

/* ---- fused FM model body: gather + LR + second-order interaction, [B,F,D] never stored ----
 * Replaces the op sequence feature_embedding.py:188-214 -> logistic_regression.py:30-35 ->
 * inner_product.py:41-48 -> factorization_machine.py:30-34 (forward and autograd backward).
 * emb[i] (dim D, all equal) and lr[i] (dim 1) describe the SAME feature i (same ids); only
 * one-id-per-sample categorical and numeric features can be fused.  Either array may be NULL
 * (lr == NULL: interaction only; emb == NULL: LogisticRegression only).
 *   d_logit[B] = sum_f lr_f + bias + 0.5 * sum_d[(sum_f e_fd)^2 - sum_f e_fd^2]
 *   d_prob[B]  = sigmoid(d_logit)  (optional, NULL to skip: the model's y_pred -- ranking_model.py output_activation --
 *                out of the same pass)
 *   d_sum[B,D] = sum_f e_f   (kept for the backward; may be NULL for inference)
 * Backward: row r of table f gets  dW[r] += sum_b g_b S_b - w_r * sum_b g_b  and
 * dW_lr[r] += sum_b g_b  over the samples b that looked r up (sorted, segmented,
 * deterministic); numeric weights and the bias are batch reductions.  Grads go into
 * emb[i].grad / lr[i].grad (dense; stored when accumulate == 0, added otherwise) and d_dbias[1].
 * phases: bit 0 = categorical tables (needs the sort), bit 1 = numeric weights + bias (does
 * not): a caller that sorts on another stream runs phase 2 first and phase 1 after the join; bit 2 = the
 * numeric-feature gradients and d_dbias are uninitialised memory: STORE them (no zero fill by the caller) instead of adding.
 * Two tiers (round 3).  Tables of up to 16 384 rows ("tier A", admitted smallest first while their gradients stay under
 * 4 MB; a rule over the tables alone, never the batch) skip the global sort: rbx_fm_sort leaves, per (feature, block of
 * 2048 samples), the block's (row, sample) pairs sorted in LDS and a bitmap of the rows present; rbx_fm_bwd sums
 * g_b S_b per (block, row), then ONE lane group per table row adds that row's block partials in ascending order and
 * WRITES the row -- every row of a tier-A table is written by every backward (zeros where nothing was looked up), so
 * these tables need no zero fill and rbx_fm_rezero skips them.  The other tables ("tier B") keep the sorted, segmented
 * path.  All sums have a fixed order: gradients are bit-identical run to run.  With bit 0 set, bit 3 (8) leaves tier A
 * out and bit 4 (16) leaves tier B out of this call: a caller with two streams runs the two tiers side by side (tier A
 * needs rbx_fm_sort_phases bits 0 and 2 done, tier B bits 0 and 1).  Calls with emb == NULL are one tier (B). */
int rbx_fm_fwd(const rbx_field_t* emb, const rbx_field_t* lr, int32_t n_fields, int64_t batch,
               const float* d_lr_bias, const float* d_extra, int32_t n_extra, int32_t extra_stride,
               int32_t extra_lr_off, const int32_t* d_extra_index, int64_t extra_rows, float* d_logit,
               float* d_prob, float* d_sum, int32_t* d_status, void* stream);
/* Rows of row-sharded tables arrive from their owners instead of being gathered locally:
 * d_extra[B, n_extra, extra_stride] holds, per (sample, table), the embedding row in floats [0, D)
 * and the dim-1 LR weight at float extra_lr_off (-1: none); they take part in S, Q and the LR sum
 * exactly like local features.  rbx_fm_extra_bwd writes their gradient block in the same packed
 * layout ([g (S - e) | g at the LR slot | 0]); it travels back to the owners (recbox_amd/sharded.py).
 * dim == 0 there means "LR weights only".
 * d_extra_index (optional, [B, n_extra] int32): d_extra is then the exchange buffer itself,
 * [extra_rows, extra_stride], and row (b, t) sits at wire slot d_extra_index[b, t] (rbx_route); a slot
 * outside [0, extra_rows) is a lookup that found no room on the wire: zero row, no gradient.  The
 * indexed rbx_fm_extra_bwd writes only the slots that are referenced: the caller zero-fills d_dextra. */
int rbx_fm_extra_bwd(const float* d_dlogit, const float* d_sum, const float* d_extra, int64_t batch,
                     int32_t n_extra, int32_t dim, int32_t extra_stride, int32_t extra_lr_off,
                     const int32_t* d_extra_index, int64_t extra_rows, float* d_dextra, void* stream);

/* ---- C1: routing of the padded, sync-free exchange of row-sharded tables (no reference precedent:
 * SURVEY.md 2.1 / 8e; layout in recbox_amd/sharded.py).  tables[t] describes the id column of sharded
 * table t (only ids / ids_stride_b / ids_dtype are read: the same strided, typed columns rbx_fm_fwd
 * takes); lookup i = b * n_tables + t.  owner = id mod world; d_base[world, n_tables] = first row of table t inside
 * the owner's packed weight; the row number base[owner][t] + id div world is written to wire slot
 * d_slot[i] = owner * capacity + (count of earlier lookups with that owner) of d_send[world * capacity]
 * (empty slots = -1).  Lookups that do not fit get slot world * capacity and set *d_overflow = 1
 * (never cleared here).  Stable and deterministic; no host sync. */
size_t rbx_route_workspace_size(int64_t n_lookups, int32_t world);
int rbx_route(const rbx_field_t* tables, int32_t n_tables, int64_t batch, int32_t world, int64_t capacity,
              const int64_t* d_base, int64_t* d_send, int32_t* d_slot, uint8_t* d_overflow, void* d_workspace,
              size_t workspace_bytes, void* stream);
/* The same with 32-bit row numbers on the wire (d_send [world * capacity] int32, empty slots = -1): the row numbers of one
 * shard fit 31 bits whenever rbx_embed_fwd can address the shard at all, and the id exchange is half as long. */
int rbx_route32(const rbx_field_t* tables, int32_t n_tables, int64_t batch, int32_t world, int64_t capacity,
                const int64_t* d_base, int32_t* d_send, int32_t* d_slot, uint8_t* d_overflow, void* d_workspace,
                size_t workspace_bytes, void* stream);

/* ---- C1 (second generation): ONE exchange each way for row-sharded tables, pooled lookups reduced at the owner
 * (csrc/rbx_shard.hip; no reference precedent -- the reference's only parallelism is nn.DataParallel / DDP, SURVEY.md
 * 2.1 -- this is SURVEY.md 5.8 / 8e and BASELINE.json configs 3 and 4).  Per sample: n_rows single-row lookups
 * (one-hot features and the columns of a pooling='concat' sequence: third_party/rechub/basic/layers.py:72,98-107) and
 * n_pool <= 1 id-masked mean / sum pooled sequence (layers.py:135-148,187-210; YoutubeDNN's history,
 * models/matching/youtube_dnn.py:46-56).  owner = id mod world, local row = d_base[owner][lookup] + id div world.
 * Static wire format per (requester, owner) pair:
 *   int32 chunk of rbx_shard_int_chunk() values: [cap_pool row numbers grouped by sample | n_pool * (batch + 1)
 *     offsets | cap_rows row numbers (-1 = empty)],
 *   fp32 chunk of rbx_shard_float_rows() rows x dim: [n_pool * batch partial sums (gradients) | cap_rows rows].
 * The all-to-alls between the calls are the caller's (recbox_amd/comm.py over RCCL, or rbx_all_to_all).
 *   rbx_shard_route        requester: ids -> d_send[world][int chunk]; d_slot[batch][n_rows] = wire slot of each
 *                          single-row lookup (owner * cap_rows + rank; world * cap_rows = did not fit / out of range);
 *                          d_inv[batch] = 1 / (valid ids + eps) (mean) or 1 (sum).  row_fields[t] / pool_field: ids,
 *                          strides, ids_dtype, vocab (+ seq_len, mask_id, pool, eps of the pooled one) are read.
 *                          Lookups beyond a capacity set *d_overflow; ids outside [0, vocab) set bit 0 of *d_status
 *                          (the reference raises IndexError) and are treated as absent.
 *   rbx_shard_serve        owner: d_recv[world][int chunk] -> d_back[world][float rows][dim] (one partial sum per
 *                          (source, sample), one row per occupied single-row slot), plus for the backward
 *                          d_keys[world * (cap_pool + cap_rows)] (local row of every received lookup, -1 = none) and
 *                          d_src (row of the gradient buffer [world * float rows, dim] holding its upstream gradient):
 *                          rbx_embed_sort over d_keys + rbx_embed_bwd_indexed(d_dout_index = d_src) is the owner's
 *                          deterministic scatter-add.  A row number >= n_local_rows sets bit 1 of *d_status.
 *   rbx_shard_combine_fwd  requester: places row (b, t) and the scaled sum of the world partial sums of sample b at
 *                          d_out + b * out_stride_b + col_off[lookup] (HOST array, n_rows + n_pool entries; the
 *                          pooled lookup is the last one): the slots of the layer's [batch, width] output block.
 *   rbx_shard_combine_bwd  requester: the upstream gradient of those slots -> d_gsend[world][float rows][dim]. */
typedef struct rbx_shard_geom {
  int32_t world;
  int32_t dim;               /* floats per row, multiple of 4 */
  int32_t n_rows;            /* single-row lookups per sample */
  int32_t n_pool;            /* pooled lookups per sample: 0 or 1 */
  int64_t batch;             /* samples per rank (equal on every rank: static wire sizes) */
  int64_t cap_rows;          /* wire slots per (requester, owner) pair for single-row lookups */
  int64_t cap_pool;          /* ... for the ids of the pooled lookup */
} rbx_shard_geom_t;
size_t rbx_shard_int_chunk(const rbx_shard_geom_t* geom);
size_t rbx_shard_float_rows(const rbx_shard_geom_t* geom);
size_t rbx_shard_route_workspace_size(const rbx_shard_geom_t* geom, int32_t pool_seq_len);
int rbx_shard_route(const rbx_shard_geom_t* geom, const rbx_field_t* row_fields, const rbx_field_t* pool_field,
                    const int64_t* d_base, int32_t* d_send, int32_t* d_slot, float* d_inv, uint8_t* d_overflow,
                    int32_t* d_status, void* d_workspace, size_t workspace_bytes, void* stream);
int rbx_shard_serve(const rbx_shard_geom_t* geom, const int32_t* d_recv, const float* d_weight, int64_t n_local_rows,
                    float* d_back, int32_t* d_keys, int32_t* d_src, int32_t* d_status, void* stream);
int rbx_shard_combine_fwd(const rbx_shard_geom_t* geom, const float* d_back, const int32_t* d_slot, const float* d_inv,
                          float* d_out, int64_t out_stride_b, const int64_t* col_off, void* stream);
int rbx_shard_combine_bwd(const rbx_shard_geom_t* geom, const float* d_dout, int64_t dout_stride_b,
                          const int64_t* col_off, const int32_t* d_slot, const float* d_inv, float* d_gsend,
                          void* stream);
size_t rbx_fm_bwd_workspace_size(const rbx_field_t* emb, const rbx_field_t* lr, int32_t n_fields, int64_t batch);
int rbx_fm_sort(const rbx_field_t* emb, const rbx_field_t* lr, int32_t n_fields, int64_t batch,
                void* d_workspace, size_t workspace_bytes, int32_t* d_status, void* stream);
/* rbx_fm_sort in pieces, for a caller that wants to order other work between them.  phases: bit 0 = id columns of any
 * dtype / stride -> the workspace's int32 [feature][batch] matrix, range-checked (d_status) -- both tiers read it; bit 1 =
 * tier B: (row, sample) pairs + segmented radix sort; bit 2 = tier A: the per-block sorts.  Bits 1 and 2 need bit 0 done
 * on the same workspace (same call or an earlier one on the same stream).  rbx_fm_sort == all three. */
int rbx_fm_sort_phases(const rbx_field_t* emb, const rbx_field_t* lr, int32_t n_fields, int64_t batch,
                       void* d_workspace, size_t workspace_bytes, int32_t* d_status, int32_t phases, void* stream);
int rbx_fm_bwd(const rbx_field_t* emb, const rbx_field_t* lr, int32_t n_fields, int64_t batch,
               const float* d_dlogit, const float* d_sum, float* d_dbias, int32_t accumulate,
               int32_t phases, void* d_workspace, size_t workspace_bytes, void* stream);
/* For a caller that keeps PERSISTENT dense gradient buffers (the reference's autograd allocates and zero-fills a new
 * [V, D] gradient per table and step: torch/nn/functional.py embedding backward; 379 MB per step at the Criteo
 * shape, of which a batch touches 36 MB): with the workspace of the PREVIOUS rbx_fm_sort (same fields, same batch)
 * and emb[i].grad / lr[i].grad = the buffers that step's rbx_fm_bwd stored into, write zeros to exactly the rows it
 * touched.  Call it before the next rbx_fm_sort reuses the workspace. */
/* (Round 4's sort-free third tier -- rbx_fm_tier_c, rbx_fm_rezero_fusable, rbx_fm_sort_phases bit 3 -- measured a draw on uniform
 * ids and a loss on skewed ones in two rounds running and was removed in round 5: docs/history/.) */
/* Round 5: rbx_fm_fwd has a second kernel (csrc/rbx_fm_quad.hip) for the wire format of the reference's ranking loader --
 * every feature's ids / values the columns, in feature order, of ONE row-major batch tensor of one dtype
 * (ranking/pytorch/dataloaders/h5_dataloader.py:36-47, ranking_model.py:106-116), dim 16, both field arrays given, the
 * tables within 4 GiB of each other, no extra rows.  Same results as the general kernel, operation for operation.  Taken
 * automatically; rbx_fm_quad(0) forces the general kernel (A/B measurements, tests), a negative value only reads; returns
 * the previous setting (RBX_FM_QUAD=0 in the environment: off from the start). */
int rbx_fm_quad(int32_t enable);
/* Round 5: the id sort behind every backward (rbx_embed_sort, rbx_fm_sort, ...) runs as 1 + passes launches when no table
 * group of the call has more than 64 sort tiles (131 072 lookups): the pairs kernel counts every pass's digit per tile, and a
 * scatter workgroup takes the start of its runs from those counts plus what the tiles in front of it publish
 * (csrc/rbx_embed_bwd.hip, BwdPlan::chained).  rbx_sort_chained(0) forces the histogram / scan / scatter launches per pass
 * for every call (A/B measurements, tests; the results are the same pairs in the same order); a negative value only reads;
 * returns the previous setting.  The workspace sizes depend on the setting: size and call with the same one. */
int rbx_sort_chained(int32_t enable);
int rbx_fm_rezero(const rbx_field_t* emb, const rbx_field_t* lr, int32_t n_fields, int64_t batch,
                  void* d_workspace, size_t workspace_bytes, void* stream);
/* rbx_fm_rezero(d_rezero_workspace) followed by rbx_fm_sort_phases(d_sort_workspace, phases = 1) -- the head of a step with
 * persistent gradients, same fields, same batch for both -- as ONE launch whose workgroups are id-compaction tiles or re-zero
 * blocks (the two share no data).  The two workspaces may be the same one (the previous sort's pairs and the compact id
 * matrix lie in different regions of the layout) or differ (the previous step's ids were sorted ahead, into a workspace of
 * the caller's).  A call without sorted tables only compacts, one without a compact matrix only clears, batch == 0 does
 * nothing.  Same stores, same status word as the two calls. */
int rbx_fm_head(const rbx_field_t* emb, const rbx_field_t* lr, int32_t n_fields, int64_t batch,
                const void* d_rezero_workspace, size_t rezero_workspace_bytes, void* d_sort_workspace,
                size_t sort_workspace_bytes, int32_t* d_status, void* stream);
/* Two lookups over the SAME id tensors with the same table layout (the embedding tables of FeatureEmbedding and the dim-1
 * tables of LogisticRegression over one batch: feature_embedding.py + logistic_regression.py:30-35) sort identical
 * (row, sample) pairs.  Given the descriptors of a sort that is already in d_src_workspace (src_is_fm = 0: src_a is an
 * rbx_embed_sort field array, src_b unused; 1: src_a / src_b are rbx_fm_sort's emb / lr arrays) and those of the lookup
 * that needs one (dst_*), copy the sorted pairs instead of sorting again.  Returns RBX_ERR_UNSUPPORTED -- nothing was
 * launched, sort as usual -- when the two do not sort the same pairs. */
int rbx_sort_share(const rbx_field_t* src_a, const rbx_field_t* src_b, int32_t src_n, int32_t src_is_fm,
                   const void* d_src_workspace, const rbx_field_t* dst_a, const rbx_field_t* dst_b, int32_t dst_n,
                   int32_t dst_is_fm, void* d_dst_workspace, size_t dst_workspace_bytes, int64_t batch, void* stream);
/* The same for the generic lookup: the rows named by the previous rbx_embed_sort on this workspace (fields[i].grad =
 * the persistent buffers its rbx_embed_bwd stored into).  Only for tables that get their gradient from that lookup alone. */
int rbx_embed_rezero(const rbx_field_t* fields, int32_t n_fields, int64_t batch, void* d_workspace,
                     size_t workspace_bytes, void* stream);

/* ---- opt-in sparse-row optimiser step (SURVEY.md 8b "or, opt-in, a sparse-row update path"; 2.2 K3).  The reference
 * runs a dense torch.optim step over dense [V, D] gradients (ranking/pytorch/models/ranking_model.py:191-197,
 * matching/pytorch/models/match_model.py:194-199).  After rbx_embed_sort + rbx_embed_bwd (rbx_fm_sort + rbx_fm_bwd) of a
 * step, the workspace still holds the sorted (row, lookup) pairs: the head of every run of equal rows names one touched row,
 * whose summed gradient sits in fields[i].grad.  These calls apply ONE optimiser step to exactly those rows of
 * fields[i].table (written in place) and of the state tensors -- same shape as the gradient, d_state1[i] / d_state2[i] per
 * feature i (HOST arrays of DEVICE pointers; features that share a table pass the same pointers):
 * with g = fields[i].grad's row + weight_decay * w for ALL three rules (L2 on the touched rows),
 *   RBX_OPT_SGD      w -= lr g
 *   RBX_OPT_ADAGRAD  state1 += g^2; w -= lr g / (sqrt(state1) + eps)          (torch.optim.Adagrad's sparse branch; the
 *                    caller folds lr_decay into lr)
 *   RBX_OPT_ADAM     state1 = beta1 state1 + (1 - beta1) g; state2 = beta2 state2 + (1 - beta2) g^2;
 *                    w -= lr state1 / (sqrt(state2) + eps)   with lr = lr0 sqrt(1 - beta2^t) / (1 - beta1^t) folded in by
 *                    the caller (torch.optim.SparseAdam: the moments of untouched rows do not decay)
 * Every row the batch looked up is stepped exactly once, whatever its summed gradient (a zero gradient still decays Adam's
 * moments and moves w by the decayed first moment, as torch.optim.SparseAdam on a coalesced gradient does).
 * Rows the batch did not touch, padding_idx rows and masked lookups are neither read nor written.  The tier-A tables of
 * the fused FM body (every row written by every backward) count a row as touched when some block's presence bitmap has it.
 * Call between the backward and the next sort on that workspace. */
typedef enum { RBX_OPT_SGD = 0, RBX_OPT_ADAGRAD = 1, RBX_OPT_ADAM = 2 } rbx_opt_kind_t;
typedef struct rbx_opt {
  int32_t kind;              /* rbx_opt_kind_t */
  float   lr;                /* effective step size (bias correction / decay folded in) */
  float   beta1, beta2;      /* Adam */
  float   eps;
  float   weight_decay;      /* L2 on the touched rows, every rule: g += weight_decay * w (0 for torch's sparse rules) */
  const float* d_step_size;  /* NULL, or a DEVICE float that overrides lr: a step captured into a hipGraph bakes every
                              * by-value argument in, so a rule whose step size depends on the step count (Adam's bias
                              * correction, Adagrad's lr_decay) reads it from memory that rbx_opt_advance updates in-graph */
} rbx_opt_t;
/* t = *d_t + 1 -> *d_t; *d_step_size = the rule's effective step size at step t: SGD lr; Adagrad lr / (1 + (t - 1) lr_decay);
 * Adam lr sqrt(1 - beta2^t) / (1 - beta1^t).  One tiny launch per optimiser step; d_t is a float counter (exact to 2^24). */
int rbx_opt_advance(int32_t kind, float lr, float beta1, float beta2, float lr_decay, float* d_t, float* d_step_size,
                    void* stream);
int rbx_embed_sparse_update(const rbx_field_t* fields, int32_t n_fields, int64_t batch, const void* d_workspace,
                            size_t workspace_bytes, const rbx_opt_t* opt, float* const* d_state1, float* const* d_state2,
                            void* stream);
int rbx_fm_sparse_update(const rbx_field_t* emb, const rbx_field_t* lr, int32_t n_fields, int64_t batch,
                         const void* d_workspace, size_t workspace_bytes, const rbx_opt_t* opt,
                         float* const* d_emb_state1, float* const* d_emb_state2, float* const* d_lr_state1,
                         float* const* d_lr_state2, void* stream);

/* ---- C2: the exchange itself on the caller's stream.  The reference has no sharded exchange (nn.DataParallel / DDP
 * only); recbox_amd/comm.py uses torch.distributed's all_to_all_single by default, which runs on RCCL's
 * own stream behind two event joins.  rbx_all_to_all is the same grouped ncclSend / ncclRecv sequence enqueued on
 * `stream`: block p of d_send (bytes_per_peer bytes) goes to rank p, block p of d_recv comes from rank p.  `comm` is
 * the ncclComm_t of the process group (ProcessGroupNCCL._comm_ptr()); rbx_comm_bind hands over the RCCL entry points
 * of the library the process has already loaded (ncclGroupStart, ncclGroupEnd, ncclSend, ncclRecv, ncclGetErrorString). */
int rbx_comm_bind(void* fn_group_start, void* fn_group_end, void* fn_send, void* fn_recv, void* fn_error_string);
int rbx_all_to_all(void* comm, const void* d_send, void* d_recv, size_t bytes_per_peer, int32_t world, void* stream);
/* The other two collectives of the sharded step the same way (round 4): the flat all-reduce of the replicated /
 * data-parallel gradients (the reference's counterpart is nn.DataParallel's gradient gather,
 * third_party/rechub/trainers/ctr_trainer.py:41-43) and the all-gather of a synchronised BatchNorm's statistics, as
 * ncclAllReduce / ncclAllGather on `stream` -- with all three on the step's own stream no collective crosses to RCCL's
 * stream, and the whole step (collectives included) is one hipGraph capture.  dtype: RBX_I32 / RBX_I64 / RBX_F32 /
 * RBX_F64; op: RBX_REDUCE_*; in place when d_send == d_recv.  rbx_comm_bind_collectives hands over ncclAllReduce and
 * (optional, NULL) ncclAllGather and ncclCommUserRank of the loaded RCCL; with the latter rbx_all_to_all moves the block
 * a rank keeps for itself by a device-to-device copy instead of RCCL's self send / recv. */
#define RBX_REDUCE_SUM 0
#define RBX_REDUCE_MAX 2
#define RBX_REDUCE_MIN 3
int rbx_comm_bind_collectives(void* fn_all_reduce, void* fn_all_gather, void* fn_comm_user_rank);
int rbx_all_reduce(void* comm, const void* d_send, void* d_recv, size_t count, int32_t dtype, int32_t op, void* stream);
int rbx_all_gather(void* comm, const void* d_send, void* d_recv, size_t bytes_per_rank, void* stream);

/* ---- K5: two-tower scoring (third_party/rechub/models/matching/dssm.py:48,57,65,
 * youtube_dnn.py:47-48,56,65,70).  l2norm = F.normalize(x, p=2, dim=-1, eps): y = x / max(||x||, eps);
 * d_inv[rows] keeps 1/max(||x||,eps) (negative when the clamp was active) for the backward.
 * pairdot: out[b,n] = scale * <u[b,:], v[b,n,:]>  (DSSM: n_cand = 1; YoutubeDNN: 1 + n_neg, scale = 1/T). */
int rbx_l2norm_fwd(const float* d_x, int64_t rows, int32_t dim, float eps, float* d_y, float* d_inv, void* stream);
/* The same over rows that sit inside a wider block: row r = (r / inner, r % inner) at d_x + (r / inner) * outer_stride +
 * (r % inner) * dim -- the [B, 1 + n_neg, D] item rows of YoutubeDNN read where the gather left them, behind the user
 * columns of one [B, width] block (youtube_dnn.py:52-70), without a contiguous copy.  d_y [rows, dim] is contiguous. */
int rbx_l2norm_fwd_strided(const float* d_x, int64_t inner, int64_t outer_stride, int64_t rows, int32_t dim, float eps,
                           float* d_y, float* d_inv, void* stream);
/* F.normalize of the candidate rows and their inner product with the (already normalised) user vector in ONE pass
 * (youtube_dnn.py:56,65,70): out[b, n] = scale * <u[b], v[b, n]> / max(|v[b, n]|, eps); d_inv[b, n] keeps 1 / max(|v|, eps)
 * (negative when the clamp was active).  The normalised rows are never materialised.  v rows at d_v + b * v_outer_stride +
 * n * dim (read where the gather left them); backward: d_du[b] = sum_n scale dout v_hat, d_dv rows (the projection of
 * scale dout u / |v| orthogonal to v_hat; plain when clamped) at d_dv + b * dv_outer_stride + n * dim. */
int rbx_cosdot_fwd(const float* d_u, const float* d_v, int64_t v_outer_stride, int64_t batch, int32_t n_cand, int32_t dim,
                   float eps, float scale, float* d_out, float* d_inv, void* stream);
int rbx_cosdot_bwd(const float* d_u, const float* d_v, int64_t v_outer_stride, const float* d_inv, const float* d_dout,
                   int64_t batch, int32_t n_cand, int32_t dim, float scale, float* d_du, float* d_dv,
                   int64_t dv_outer_stride, void* stream);
int rbx_l2norm_bwd(const float* d_y, const float* d_inv, const float* d_dy, int64_t rows, int32_t dim,
                   float* d_dx, void* stream);
int rbx_pairdot_fwd(const float* d_u, const float* d_v, int64_t batch, int32_t n_cand, int32_t dim, float scale,
                    float* d_out, void* stream);
int rbx_pairdot_bwd(const float* d_u, const float* d_v, const float* d_dout, int64_t batch, int32_t n_cand,
                    int32_t dim, float scale, float* d_du, float* d_dv, void* stream);

/* ---- BatchNorm1d of the dense towers (third_party/rechub/basic/layers.py:255-263: Linear -> BatchNorm1d ->
 * activation -> Dropout after every layer; optional in core/pytorch/layers/mlp.py:25-37 and
 * ranking/pytorch/layers/blocks/mlp_block.py:42-58).  x [rows, cols] row-major, statistics per column.
 * training != 0: batch statistics (biased variance normalises, the running statistics receive
 * (1 - momentum) * old + momentum * {mean, unbiased variance} when the pointers are given); training == 0:
 * running statistics.  d_mean / d_rstd [cols] are outputs kept for the backward.  relu != 0 applies ReLU to y;
 * the backward then takes that y as d_y_relu (mask y > 0) -- NULL when no activation was fused.
 * Backward: d_dgamma = sum dy * xhat, d_dbeta = sum dy (always written, also used as scratch),
 * d_dx = gamma * rstd * (dy - dbeta/M - xhat * dgamma/M) (training) or gamma * rstd * dy (eval); NULL skips it.
 * Reductions are two-stage in a fixed order (Welford partials merged with Chan's formula): deterministic.
 * Alignment: none is required of any pointer beyond that of a float.  The element-wise passes take their float4 form
 * when cols % 4 == 0 and x, y (forward) or x, dy, dx and d_y_relu (backward) are all 16-byte aligned, the scalar form
 * otherwise; the results are the same. */
size_t rbx_batchnorm_workspace_size(int64_t rows, int32_t cols);
int rbx_batchnorm_fwd(const float* d_x, int64_t rows, int32_t cols, const float* d_gamma, const float* d_beta, float eps,
                      int32_t training, float momentum, float* d_running_mean, float* d_running_var, int32_t relu,
                      float* d_mean, float* d_rstd, float* d_y, void* d_workspace, size_t workspace_bytes, void* stream);
int rbx_batchnorm_bwd(const float* d_x, const float* d_dy, const float* d_y_relu, int64_t rows, int32_t cols,
                      const float* d_gamma, const float* d_mean, const float* d_rstd, int32_t training, float* d_dx,
                      float* d_dgamma, float* d_dbeta, void* d_workspace, size_t workspace_bytes, void* stream);

/* nn.PReLU behind the BatchNorm of a tower layer (rechub MLP with activation="prelu": Linear -> BatchNorm1d -> PReLU ->
 * Dropout, third_party/rechub/basic/layers.py:255-263, activation.py:44-45; DSSM's towers in BASELINE cfg 1) in the same
 * passes: y = z > 0 ? z : a z on the normalised value z, a = d_slope[0] (slope_n == 1: nn.PReLU()) or one per column
 * (slope_n == cols).  Backward rebuilds z from x (its sign is the mask -- y's is not when a <= 0):
 * dz = z > 0 ? dy : a dy, d_dslope_cols[c] = sum dy z over z <= 0 (sum it over c for the single-parameter form). */
int rbx_batchnorm_prelu_fwd(const float* d_x, int64_t rows, int32_t cols, const float* d_gamma, const float* d_beta,
                            const float* d_slope, int32_t slope_n, float eps, int32_t training, float momentum,
                            float* d_running_mean, float* d_running_var, float* d_mean, float* d_rstd, float* d_y,
                            void* d_workspace, size_t workspace_bytes, void* stream);
int rbx_batchnorm_prelu_bwd(const float* d_x, const float* d_dy, int64_t rows, int32_t cols, const float* d_gamma,
                            const float* d_beta, const float* d_slope, int32_t slope_n, const float* d_mean,
                            const float* d_rstd, int32_t training, float* d_dx, float* d_dgamma, float* d_dbeta,
                            float* d_dslope_cols, void* d_workspace, size_t workspace_bytes, void* stream);
/* The same in pieces, for a SYNCHRONISED BatchNorm over the ranks of a data-parallel job (torch.nn.SyncBatchNorm: RecBole's
 * DDP path converts every BatchNorm of the model, third_party/recbole/trainer/trainer.py:60-64; rechub's nn.DataParallel
 * keeps per-replica statistics, ctr_trainer.py:43 -- the default here).  The caller's collectives sit between the calls:
 *   rbx_batchnorm_stats       d_raw[3, cols] = this rank's (count, mean, M2 = sum (x - mean)^2) per column;
 *                             all-gather, merge (Chan), derive mean / rstd and the running statistics;
 *   rbx_batchnorm_apply       y = (x - mean) rstd gamma + beta (+ ReLU) with the GLOBAL d_mean / d_rstd;
 *   rbx_batchnorm_bwd_reduce  this rank's d_dgamma = sum dy xhat, d_dbeta = sum dy (the parameter gradients: the job's
 *                             gradient all-reduce sums them over the ranks like every other replicated parameter);
 *                             all-reduce a COPY of the two for the next call;
 *   rbx_batchnorm_bwd_dx      dx = gamma rstd (dy - dbeta / N - xhat dgamma / N) with the GLOBAL sums and
 *                             N = total_rows = rows of all ranks together. */
int rbx_batchnorm_stats(const float* d_x, int64_t rows, int32_t cols, float* d_raw, void* d_workspace,
                        size_t workspace_bytes, void* stream);
int rbx_batchnorm_apply(const float* d_x, int64_t rows, int32_t cols, const float* d_gamma, const float* d_beta,
                        const float* d_mean, const float* d_rstd, int32_t relu, float* d_y, void* stream);
int rbx_batchnorm_bwd_reduce(const float* d_x, const float* d_dy, const float* d_y_relu, int64_t rows, int32_t cols,
                             const float* d_mean, const float* d_rstd, float* d_dgamma, float* d_dbeta, void* d_workspace,
                             size_t workspace_bytes, void* stream);
int rbx_batchnorm_bwd_dx(const float* d_x, const float* d_dy, const float* d_y_relu, int64_t rows, int32_t cols,
                         const float* d_gamma, const float* d_mean, const float* d_rstd, const float* d_dgamma,
                         const float* d_dbeta, int64_t total_rows, float* d_dx, void* stream);

/* ---- xDeepFM's CIN outer product (ranking/pytorch/layers/interactions/compressed_interaction_net.py:35-48; csrc/rbx_cin.hip):
 * d_z[(b, d), h * m + j] = x0[b, h, d] * xk[(b, d), j], rows = batch * dim, in the A layout of the GEMM that runs the 1x1
 * Conv1d over the channel axis.  d_x0 [batch, n_fields, dim] (the embedding layer's output as it is); d_xk [batch * dim, m]
 * (the previous layer's GEMM output as it is) or NULL for the first layer (X_k = X_0, m == n_fields).  Backward: d_dx0
 * [batch, n_fields, dim] (both uses of X_0 when d_xk is NULL) and d_dxk [batch * dim, m]; NULL skips either. */
int rbx_cin_outer_fwd(const float* d_x0, const float* d_xk, int64_t batch, int32_t n_fields, int32_t m, int32_t dim,
                      float* d_z, void* stream);
int rbx_cin_outer_bwd(const float* d_x0, const float* d_xk, const float* d_dz, int64_t batch, int32_t n_fields, int32_t m,
                      int32_t dim, float* d_dx0, float* d_dxk, void* stream);

/* ---- the towers' activations that are not fused into a GEMM epilogue or a BatchNorm pass (csrc/rbx_act.hip; round 5).
 * x, y, dy, dx: [rows, cols] row-major f32.  rbx_act_workspace_size: bytes for the column reductions of the calls that take a
 * workspace (partials per block of 256 rows, merged in block order: results repeat bit for bit).
 * nn.PReLU standing alone (core/pytorch/layers/mlp.py:25-37, ranking/pytorch/layers/blocks/mlp_block.py:42-58 with
 *   hidden_activations="PReLU" and no BatchNorm in front): n_slope = 1 or cols; backward dx = dy (x > 0 ? 1 : a) and
 *   d_dslope[n_slope] = sum dy x [x <= 0] (NULL skips either).
 * nn.Dropout(p), training (the same towers' dropout_rates, third_party/rechub/basic/layers.py:255-263): y = x keep / (1 - p)
 *   with keep(i) a counter-based function of (seed + *d_seed_add, i) (Philox4x32-10) -- the SAME call on dy is the backward,
 *   nothing is stored; not torch's random stream: equal in distribution to the reference, not bit for bit.
 * Dice (core/pytorch/layers/activations.py:23-33): p = sigmoid((x - mean) rstd) with the statistics of a non-affine
 *   BatchNorm1d (training: batch statistics, biased variance, running statistics updated with `momentum` when given;
 *   evaluation: the running statistics), y = p x + alpha (1 - p) x, alpha [cols].  d_mean / d_rstd [cols] are outputs kept for
 *   the backward, which returns dx (through the statistics too, in training) and d_dalpha[cols] (NULL skips either). */
size_t rbx_act_workspace_size(int64_t rows, int32_t cols);
int rbx_prelu_fwd(const float* d_x, int64_t rows, int32_t cols, const float* d_slope, int32_t n_slope, float* d_y,
                  void* stream);
int rbx_prelu_bwd(const float* d_x, const float* d_dy, int64_t rows, int32_t cols, const float* d_slope, int32_t n_slope,
                  float* d_dx, float* d_dslope, void* d_workspace, size_t workspace_bytes, void* stream);
int rbx_dropout(const float* d_x, int64_t n, float p, uint64_t seed, const uint64_t* d_seed_add, float* d_y, void* stream);
int rbx_dice_fwd(const float* d_x, int64_t rows, int32_t cols, const float* d_alpha, float eps, int32_t training,
                 float momentum, float* d_running_mean, float* d_running_var, float* d_mean, float* d_rstd, float* d_y,
                 void* d_workspace, size_t workspace_bytes, void* stream);
int rbx_dice_bwd(const float* d_x, const float* d_dy, int64_t rows, int32_t cols, const float* d_alpha, const float* d_mean,
                 const float* d_rstd, int32_t training, float* d_dx, float* d_dalpha, void* d_workspace,
                 size_t workspace_bytes, void* stream);

/* ---- LayerNorm over the last dimension (the five nn.LayerNorm(D, eps=1e-8) of a SASRec block stack,
 * third_party/rechub/models/matching/sasrec.py:52-63,81-94).  x [rows, dim] contiguous; biased variance, eps inside
 * the square root (torch semantics); d_mean / d_rstd [rows] are kept for the backward.  Backward:
 * dx = rstd * (g - mean_d(g) - xhat * mean_d(g * xhat)) with g = dy * gamma (NULL skips it);
 * d_dgamma = sum_rows dy * xhat, d_dbeta = sum_rows dy (both or neither; two-stage fixed-order reduction). */
int rbx_layernorm_fwd(const float* d_x, int64_t rows, int32_t dim, const float* d_gamma, const float* d_beta, float eps,
                      float* d_mean, float* d_rstd, float* d_y, void* stream);
size_t rbx_layernorm_bwd_workspace_size(int64_t rows, int32_t dim);
int rbx_layernorm_bwd(const float* d_x, const float* d_dy, int64_t rows, int32_t dim, const float* d_gamma,
                      const float* d_mean, const float* d_rstd, float* d_dx, float* d_dgamma, float* d_dbeta,
                      void* d_workspace, size_t workspace_bytes, void* stream);

/* ---- K7: candidate scoring without materialising the candidate embeddings
 * (third_party/rechub/models/matching/sasrec.py:98-105: pos/neg logits = (seq_output * item_emb(ids)).sum(-1);
 * the [rows, 1 + n] sampled-softmax logits consumed by core/pytorch/losses/softmax_crossentropy_loss.py:14-22).
 *   d_out[r, c] = scale * < d_x[r, :], table_c[ids_c[r], :] >
 * cands[i] is one candidate set: ids ([rows] or [rows, seq_len] through ids_stride_b / ids_stride_l, any id
 * dtype), table/vocab/dim (all sets share dim), seq_len = candidates per row, out_off = first output column;
 * the sets together must cover columns [0, n_out) exactly once (n_out <= 256).  Out-of-range ids score 0 and
 * raise d_status.  Backward: dense dW into cands[i].grad through the sorted segmented scatter-add
 * (contribution scale * g[r,c] * x[r,:]; rows equal to padding_idx receive no gradient; grad == NULL =
 * frozen), and d_dx[r, :] = scale * sum_c g[r,c] * row (skipped when d_dx is NULL).  rbx_gatherdot_sort
 * depends on the ids only and may run on another stream during the forward. */
int rbx_gatherdot_fwd(const rbx_field_t* cands, int32_t n_cands, int64_t rows, const float* d_x, int64_t x_stride,
                      float scale, float* d_out, int32_t* d_status, void* stream);
size_t rbx_gatherdot_bwd_workspace_size(const rbx_field_t* cands, int32_t n_cands, int64_t rows);
int rbx_gatherdot_sort(const rbx_field_t* cands, int32_t n_cands, int64_t rows, void* d_workspace,
                       size_t workspace_bytes, int32_t* d_status, void* stream);
int rbx_gatherdot_bwd(const rbx_field_t* cands, int32_t n_cands, int64_t rows, const float* d_x, int64_t x_stride,
                      const float* d_dout, float scale, float* d_dx, int64_t dx_stride, int32_t accumulate,
                      void* d_workspace, size_t workspace_bytes, void* stream);

/* ---- the two-tower loader's per-epoch negative sampling and per-batch item-corpus gather
 * (matching/pytorch/dataloaders/h5_generator.py:61-84 sampling_block, :144-181 negative_sampling,
 * :23-28 TrainDataset.__getitem__, :49-58 collate_fn).
 * rbx_negsample: d_out[rows, (d_pos ? 1 : 0) + num_negs]; column 0 = d_pos[r] when given (hstack([pos, negs]));
 * every other entry is uniform over [0, num_items) with replacement (np.random.choice(..., replace=True)).
 * With d_excl_offsets/d_excl_items (CSR over queries, items sorted ascending inside a query) and d_query[rows]
 * (query of each row), items the query interacted with are never drawn (ignore_pos_items=True: uniform over
 * the complement: up to 64 redraws, then ONE exact draw of the k-th non-excluded item, so a query that interacted with
 * almost the whole corpus never receives one of its own items).  Generator: Philox4x32-10, key = seed, counter =
 * (offset + r * num_negs + j, attempt); item = high 64 bits of (low 64 random bits) x num_items.  Same (seed, offset) ->
 * same draws.  rbx_negsample_checked also bounds-checks d_query[r] against n_queries (rows of the CSR): an index outside
 * [0, n_queries) sets *d_status (numpy raises IndexError) and draws without exclusion. */
int rbx_negsample(int64_t num_items, int64_t rows, int32_t num_negs, uint64_t seed, uint64_t offset,
                  const int64_t* d_pos, const int64_t* d_query, const int64_t* d_excl_offsets,
                  const int64_t* d_excl_items, int64_t* d_out, void* stream);
int rbx_negsample_checked(int64_t num_items, int64_t rows, int32_t num_negs, uint64_t seed, uint64_t offset,
                          const int64_t* d_pos, const int64_t* d_query, const int64_t* d_excl_offsets,
                          const int64_t* d_excl_items, int64_t n_queries, int32_t* d_status, int64_t* d_out, void* stream);
/* rbx_gather_rows: for every column c and index q: dst_c[q, :] = src_c[d_index[q], :] (row_bytes bytes, any
 * element type: ids, sequences [n_items, L], float features) -- the byte-exact equivalent of
 * dict((k, v[item_indexes]) for k, v in item_corpus.items()) followed by flatten(end_dim=1).  An index outside
 * [0, n_src_rows) raises d_status (numpy raises IndexError) and reads row 0. */
typedef struct rbx_rowcopy {
  const void* src;     /* [n_src_rows, row_bytes] */
  void* dst;           /* [n_index, row_bytes] */
  int64_t row_bytes;
} rbx_rowcopy_t;
int rbx_gather_rows(const rbx_rowcopy_t* cols, int32_t n_cols, const int64_t* d_index, int64_t n_index,
                    int64_t n_src_rows, int32_t* d_status, void* stream);

/* ---- exact top-k retrieval for evaluation (core/metrics.py:54-68 evaluate_block,
 * utils/ann/faiss.py:3-15 IndexFlatIP.search).  The score matrix U I^T comes from rbx_linear_fwd (fp32 MFMA).
 * rbx_topk: for every row the k (<= 1024) largest of d_scores[r, 0..n) sorted by (score descending, column
 * ascending -- ties are deterministic, the reference leaves them to faiss/numpy); d_index (optional, same
 * layout as d_scores, any int64 values) supplies the id reported for each column, otherwise the column itself.
 * n < 2^32 - 1.  Rows shorter than k are padded with (-FLT_MAX, -1) like faiss, after every score of the row (-inf
 * included).  +0.0 and -0.0 are equal scores and either may be returned as +0.0; NaN scores have no defined place.
 * Rows longer than 16 384 scores
 * (workspace): a threshold estimated from 8 192 samples of the row, one filtering sweep, exact selection among the
 * candidates; rows the estimate cannot serve fall back, on the device, to an exact selection in several levels.
 * rbx_penalize_members: scores[r, j] = (float)((double)scores[r, j] + penalty) where candidates[r, j] is in the
 * sorted CSR list offsets/items of query d_query[r]  (mask train items: "scores += -1e9 * mask").
 * rbx_membership: flags[r, j] = candidates[r, j] in the list of d_query[r]  (hits against valid_user2items). */
size_t rbx_topk_workspace_size(int64_t rows, int64_t n, int32_t k);
int rbx_topk(const float* d_scores, const int64_t* d_index, int64_t rows, int64_t n, int64_t row_stride, int32_t k,
             float* d_out_scores, int64_t* d_out_index, void* d_workspace, size_t workspace_bytes, void* stream);
int rbx_penalize_members(const int64_t* d_candidates, int64_t rows, int32_t k, const int64_t* d_query,
                         const int64_t* d_offsets, const int64_t* d_items, double penalty, float* d_scores,
                         void* stream);
int rbx_membership(const int64_t* d_candidates, int64_t rows, int32_t k, const int64_t* d_query,
                   const int64_t* d_offsets, const int64_t* d_items, uint8_t* d_flags, void* stream);

/* rbx_search_ip: IndexFlatIP.search as one fused op -- for every user row the k (<= 1024) items with the largest
 * inner product d_users[r, :] . d_items[i, :] (fp32 products and accumulation on the fp32 MFMA, 1 <= dim <= 512),
 * without writing the [rows, n_items] score matrix: the scores of 8 192 strided sample items give a per-row
 * threshold, ONE sweep of the score kernel over all items keeps (in its epilogue, from the accumulator registers)
 * the (score, item) pairs at or above it, and rbx_topk's exact selection runs among those <= 8 192 candidates.
 * d_users: row r at d_users + r * user_stride (>= dim); d_items: [n_items, dim] contiguous; neither needs 16-byte
 * alignment.  d_row_state[r] = 1: row r of the outputs is final -- the k largest scores sorted by (score descending,
 * item index ascending), the order of rbx_topk.  d_row_state[r] = 0: the row was not served (fewer than k candidates,
 * or an overflow from ties / a skewed sample) and its outputs are unspecified: the caller computes it through
 * rbx_linear_fwd + rbx_topk.  Nothing synchronises the device; everything runs on `stream`.
 * Unsupported (rbx_search_ip_workspace_size returns 0, rbx_search_ip returns RBX_ERR_UNSUPPORTED): n_items <= 16 384
 * or k not selective (rbx_topk's sample-rank rule), k > 1024, n_items >= 2^31, dim outside [1, 512]. */
size_t rbx_search_ip_workspace_size(int64_t rows, int64_t n_items, int32_t dim, int32_t k);
int rbx_search_ip(const float* d_users, int64_t rows, int64_t user_stride, const float* d_items, int64_t n_items,
                  int32_t dim, int32_t k, float* d_out_scores, int64_t* d_out_index, int32_t* d_row_state,
                  void* d_workspace, size_t workspace_bytes, void* stream);

/* ---- cross layers (ranking/pytorch/layers/interactions/cross_net.py:22-59).
 * out = xi + x0 * h + bias:  CrossNetV2: h = Linear_i(xi) [rows, dim] (h_cols == dim, bias NULL);
 * CrossNet: h = xi w_i [rows, 1] (h_cols == 1) and bias[dim].  The Linear itself is rbx_linear_fwd.
 * Backward of the element-wise tail: d_dx0 = dout * h (NULL skips it), d_dh = dout * x0 (summed over the row when
 * h_cols == 1); d(xi) is dout itself and d(bias) its column sum. */
int rbx_cross_fwd(const float* d_x0, const float* d_xi, const float* d_h, const float* d_bias, int64_t rows, int32_t dim,
                  int32_t h_cols, float* d_out, void* stream);
int rbx_cross_bwd(const float* d_x0, const float* d_h, const float* d_dout, int64_t rows, int32_t dim, int32_t h_cols,
                  float* d_dx0, float* d_dh, void* stream);
/* out[r, :] = (alpha * x[r, :] + add[r, :]) * scale[r]   (add optional): SASRec's embedding prologue `e *= sqrt(D);
 * e += position_emb(...); e *= ~timeline_mask.unsqueeze(-1)` and its per-block mask (third_party/rechub/models/matching/
 * sasrec.py:68-77, 92) in one pass; its backward is the same call on the incoming gradient.  No alignment is required:
 * the float4 form runs when dim % 4 == 0 and d_x, d_add and d_out are 16-byte aligned, the scalar form otherwise (a
 * contiguous view one float into its storage), with the same values.  rows % add_rows != 0 and a NULL d_add of
 * rbx_rowscale_seq are RBX_ERR_INVALID. */
int rbx_rowscale(const float* d_x, const float* d_add, const float* d_scale, int64_t rows, int32_t dim, float alpha,
                 float* d_out, void* stream);
/* The same prologue with the position rows read in place: sasrec.py:68-77 looks up positions = tile(arange(L), [B, 1]), i.e.
 * the table's first L rows for every sequence.  rbx_rowscale_seq: d_add holds add_rows rows of `dim` floats that repeat every
 * add_rows rows of x (rows % add_rows == 0).  rbx_seq_colsum: the gradient of those rows,
 *   out[l, :] = sum_b scale[b * seq_len + l] * g[b, l, :]        (g [batch, seq_len, dim], out [seq_len, dim], overwritten),
 * one streaming pass + a fixed-order sum of per-32-sequence partials (deterministic); the reference's embedding backward
 * (index_add over B * L position ids) gives the same sums. */
int rbx_rowscale_seq(const float* d_x, const float* d_add, int64_t add_rows, const float* d_scale, int64_t rows, int32_t dim,
                     float alpha, float* d_out, void* stream);
size_t rbx_seq_colsum_workspace_size(int64_t batch, int32_t seq_len, int32_t dim);
int rbx_seq_colsum(const float* d_g, const float* d_scale, int64_t batch, int32_t seq_len, int32_t dim, float* d_out,
                   void* d_workspace, size_t workspace_bytes, void* stream);
/* out[r, c] = base[r, c] + (c < prefix_cols ? a[r, c] + b[r, c] : 0) for c < cols; base, a, b optional (NULL = zeros),
 * strides in floats.  The input gradient of a row block that one consumer reads whole and two more read through its
 * leading columns: DeepFM feeds the same embeddings to the tower (embeddings | dense values), to FM and to the
 * first-order Linear (third_party/rechub/models/ranking/deepfm.py:34-39; autograd's glue for it is a fill, a strided
 * copy and two adds).
 * Only out[r, 0 .. cols) is written, in every form: columns at or beyond `cols` of a row -- the padding of a stride
 * rounded up to a float4 included -- keep what they held, and nothing at or beyond `cols` (`prefix_cols` for a, b) is
 * read, so every operand may be a column view of a wider buffer.  The float4 form needs 16-byte aligned pointers,
 * prefix_cols % 4 == 0 and strides that are multiples of 4 and at least cols rounded up to 4 (out, base); anything else
 * runs the scalar form with the same values.  A stride shorter than its row, prefix_cols > cols and negative sizes are
 * RBX_ERR_INVALID; rows == 0 or cols == 0 returns at once. */
int rbx_sum_prefix(const float* d_base, int64_t base_stride, const float* d_a, int64_t a_stride, const float* d_b,
                   int64_t b_stride, int64_t rows, int32_t cols, int32_t prefix_cols, float* d_out, int64_t out_stride,
                   void* stream);

/* ---- the ranking harness's loss: F.binary_cross_entropy(y_pred, y_true, reduction='mean') on sigmoid outputs
 * (ranking/pytorch/models/ranking_model.py:69, ranking/pytorch/torch_utils.py:54-65).  torch semantics: both log terms
 * clamped at -100; d_loss[1] = mean; backward d_dprob = d_dloss[0] / n * (p - y) / max(p (1 - p), 1e-12).
 * Block partials + fixed-order final sum: deterministic. */
size_t rbx_bce_workspace_size(int64_t n);
int rbx_bce_mean_fwd(const float* d_prob, const float* d_target, int64_t n, float* d_loss, void* d_workspace,
                     size_t workspace_bytes, void* stream);
int rbx_bce_mean_bwd(const float* d_prob, const float* d_target, const float* d_dloss, int64_t n, float* d_dprob,
                     void* stream);
/* The same loss on LOGITS with both backward steps folded in (a step that owns its loss, recbox_amd.graph.ShardedFMStep):
 * p = sigmoid(x) (optional output d_prob = the model's y_pred, ranking_model.py forward), d_loss[0] = the mean BCE as above,
 * d_dlogit = grad_scale * dL/dx = grad_scale / n * (p - y) / max(p (1 - p), 1e-12) * (1 - p) p (optional). */
int rbx_sigmoid_bce_mean(const float* d_logit, const float* d_target, int64_t n, float grad_scale, float* d_prob,
                         float* d_loss, float* d_dlogit, void* d_workspace, size_t workspace_bytes, void* stream);
/* The same in ONE launch: the workgroup that finishes last adds the block partials (same fixed order, so the same bits as the
 * two-launch form).  d_counter[1] is caller-owned state that must be 0 before the first call; every call leaves it at 0.
 * Calls that share a counter must not overlap (one counter per stream). */
int rbx_sigmoid_bce_mean_onepass(const float* d_logit, const float* d_target, int64_t n, float grad_scale, float* d_prob,
                                 float* d_loss, float* d_dlogit, void* d_workspace, size_t workspace_bytes,
                                 uint32_t* d_counter, void* stream);
/* y[i] = scalar[0] * x[i], the scalar read on the device: the backward of a loss whose dL/dlogit (for an upstream gradient
 * of 1) was already written by rbx_sigmoid_bce_mean in the forward -- autograd's upstream scalar is applied without a
 * host read (ops.binary_cross_entropy on the output of ops.sigmoid_output). */
int rbx_scale_by_scalar(const float* d_x, const float* d_scalar, int64_t n, float* d_y, void* stream);

/* ---- dense tower: y = act(x W^T + b) on the fp32 matrix cores (v_mfma_f32_32x32x2_f32) -------
 * core/pytorch/layers/mlp.py:25-37, ranking/pytorch/layers/blocks/mlp_block.py:42-58,
 * third_party/rechub/basic/layers.py:255-263.  x[m,k] with row stride x_stride >= k floats (a column block of
 * a wider activation, e.g. the embedding part of a padded [B, width] gather output, is read in place),
 * W[n,k] (nn.Linear layout), bias[n] or NULL, act: 0 none, 1 ReLU.  Backward: dx[m,k] (row stride dx_stride;
 * NULL to skip), dW[n,k], db[n] (NULL to skip) are OVERWRITTEN; d_y (forward output) is only read when
 * act == 1.  Rows that are 16-byte aligned (pointer and stride) are loaded as float4. */
int rbx_linear_fwd(const float* d_x, int64_t x_stride, const float* d_w, const float* d_bias, int64_t m, int32_t n,
                   int32_t k, int32_t act, float* d_y, void* stream);
size_t rbx_linear_bwd_workspace_size(int64_t m, int32_t n, int32_t k, int32_t act);
int rbx_linear_bwd(const float* d_x, int64_t x_stride, const float* d_w, const float* d_y, const float* d_dy, int64_t m,
                   int32_t n, int32_t k, int32_t act, float* d_dx, int64_t dx_stride, float* d_dw, float* d_db,
                   void* d_workspace, size_t workspace_bytes, void* stream);
/* The same contraction with the element-wise neighbours of a transformer sub-layer folded into the epilogue, so that none
 * of them is a pass of its own over an [m, n] activation (third_party/rechub/models/matching/sasrec.py:81-94: the residual
 * `Q + mha_outputs`, `seqs *= ~timeline_mask`; in the backward, the sum autograd forms for a tensor with two readers and
 * the ReLU backward of the FFN's hidden layer):
 *   rbx_linear_fwd_fused:  y[m,n]  = (act(x W^T + b) + residual) * row_scale[row]       residual, row_scale optional (NULL)
 *   rbx_linear_dx_fused:   dx[m,k] = ((dy W) o [mask > 0]) + residual                   mask [m,k], residual [m,k] optional
 * Every operand has its own row stride (floats).  n > 1 (k > 1 for dx): the logit-head kernels have no such tail. */
int rbx_linear_fwd_fused(const float* d_x, int64_t x_stride, const float* d_w, const float* d_bias, int64_t m, int32_t n,
                         int32_t k, int32_t act, const float* d_residual, int64_t residual_stride,
                         const float* d_row_scale, float* d_y, int64_t y_stride, void* stream);
int rbx_linear_dx_fused(const float* d_dy, int64_t dy_stride, const float* d_w, int64_t m, int32_t n, int32_t k,
                        const float* d_mask, int64_t mask_stride, const float* d_residual, int64_t residual_stride,
                        float* d_dx, int64_t dx_stride, void* stream);
/* The `seqs *= ~timeline_mask` of a SASRec block (sasrec.py:92) in the backward of the Linear in front of it, without a pass
 * that writes the scaled gradient g = diag(row_scale) dy:
 *   rbx_linear_dx_scaled:   dx[m,k] = (((dy W) o [mask > 0]) + residual) * row_scale[row]
 *   rbx_linear_dwdb_scaled: dW[n,k] = g^T x, db[n] = column sums of g (d_db may be NULL); workspace as rbx_linear_bwd's with
 *                           act = 0.  RBX_ERR_UNSUPPORTED unless n = k = 64, m >= 8192 and the rows are 16-byte aligned (the
 *                           slab kernel, tall_dw64_kernel): the caller then forms g itself (rbx_rowscale) and calls rbx_linear_bwd. */
int rbx_linear_dx_scaled(const float* d_dy, int64_t dy_stride, const float* d_w, int64_t m, int32_t n, int32_t k,
                         const float* d_mask, int64_t mask_stride, const float* d_residual, int64_t residual_stride,
                         const float* d_row_scale, float* d_dx, int64_t dx_stride, void* stream);
int rbx_linear_dwdb_scaled(const float* d_x, int64_t x_stride, const float* d_dy, int64_t dy_stride, const float* d_row_scale,
                           int64_t m, int32_t n, int32_t k, float* d_dw, float* d_db, void* d_workspace,
                           size_t workspace_bytes, void* stream);
/* DeepFM (third_party/rechub/models/ranking/deepfm.py:34-42): one gathered block x [m, k] = [F * D embeddings | dense values] feeds
 * the tower's first Linear, the FM term over its leading fm_cols = F * D columns and the first-order Linear over the same
 * columns.  rbx_fm_sum_fwd: y_fm[b] = 0.5 sum_d (S_d^2 - sum_f e_fd^2) and S[b, d] = sum_f e[b, f, d] in one pass.
 * rbx_linear_dx_deepfm: the block's WHOLE gradient out of the tower's dx GEMM --
 *   dx[b, c] = sum_j dy[b, j] W[j, c]  +  [c < fm_cols] (g_fm[b] (S[b, c % fm_dim] - x[b, c]) + g_lr[b] lr_w[c])
 * instead of three kernels writing three [m, fm_cols] gradients and a fourth adding them (d_lr_g / d_lr_w may be NULL). */
int rbx_fm_sum_fwd(const float* d_emb, int64_t emb_stride_b, int64_t batch, int32_t n_fields, int32_t dim, float* d_out,
                   float* d_sum, void* stream);
/* ... with the first-order Linear over the same n_fields * dim columns in the same pass (third_party/rechub/models/ranking/
 * deepfm.py:37: LR reads the block FM reads): d_lr_out[b] = <x[b, :n_fields * dim], d_lr_w> + d_lr_b[0] (d_lr_b may be NULL). */
int rbx_fm_sum_lr_fwd(const float* d_emb, int64_t emb_stride_b, int64_t batch, int32_t n_fields, int32_t dim, float* d_out,
                      float* d_sum, const float* d_lr_w, const float* d_lr_b, float* d_lr_out, void* stream);
int rbx_linear_dx_deepfm(const float* d_dy, int64_t dy_stride, const float* d_w, int64_t m, int32_t n, int32_t k,
                         const float* d_x, int64_t x_stride, const float* d_fm_sum, int32_t fm_dim, int32_t fm_cols,
                         const float* d_fm_g, const float* d_lr_g, const float* d_lr_w, float* d_dx, int64_t dx_stride,
                         void* stream);

/* f32 GEMM on the bf16 matrix cores (csrc/rbx_dense.hip, gemm_bx6_kernel): a weight matrix split ONCE per call into three
 * bf16 planes w = h + m + l (|w - h - m - l| <= 2^-24 |w|), the activations split inside the kernel, six bf16 MFMA products
 * per f32 product with f32 accumulation -- results at f32 rounding level (the same test tolerances), ~2.7x fewer matrix-core
 * cycles than v_mfma_f32_32x32x2_f32.  (rbx_linear_bwd's weight gradient dW = dy^T x takes the same route on its own when the
 * batch has >= 8192 rows: both operands are activations, split inside gemm_bxt_kernel; RBX_GEMM_BX6=0 keeps it, too, on f32 MFMAs.)
 * No counterpart in the reference (its nn.Linear is one torch call):
 *   rbx_split_bf16_size(rows, cols, transpose): bytes of the planes of a [rows, cols] matrix;
 *   rbx_split_bf16: d_out[r][c / 8][q][c % 8] (q = 0..2 = h, m, l; c < cols rounded up to 32, zero-filled; transpose != 0:
 *                   out row r is COLUMN r of d_src) -- an opaque layout for the kernel's tile loads; transpose = 0 serves
 *                   y = x W^T (rbx_linear_fwd*), 1 serves dx = dy W (rbx_linear_dx*);
 *   rbx_split_register(d_w, d_planes, rows, cols, transposed): from now on a rbx_linear_fwd* / rbx_linear_dx* call whose
 *                   weight pointer is d_w (shape [rows, cols]) runs on the planes; rbx_split_unregister(d_w) ends that (the
 *                   planes must stay valid until the GEMMs issued in between have run).  Host-side table, 256 slots,
 *                   thread-safe; RBX_GEMM_BX6=0 in the environment ignores every registration. */
size_t rbx_split_bf16_size(int32_t rows, int32_t cols, int32_t transpose);
int rbx_split_bf16(const float* d_src, int64_t ld, int32_t rows, int32_t cols, int32_t transpose, void* d_out, void* stream);
int rbx_split_register(const float* d_w, const void* d_planes, int32_t rows, int32_t cols, int32_t transposed);
int rbx_split_unregister(const float* d_w);
uint64_t rbx_gemm_bx6_count(void);      /* GEMM calls that ran on the split-operand kernel so far (tests, logs) */

/* ---- K6: fused masked-softmax attention, any sequence length (head_dim in {4, 8, 16, 32, 64}): no explicit mask,
 * lq == lk <= 256 and head_dim 32 / 64 run on the matrix cores, everything else on the VALU kernels that stream the keys
 * through LDS in chunks (round 5: the LDS-residency limit of rounds 1-4 is gone) ----
 * ranking/pytorch/layers/attentions/dot_product_attention.py:31-43 (ScaledDotProductAttention) and the
 * attention core of nn.MultiheadAttention in third_party/rechub/models/matching/sasrec.py:81-87.
 * q[bh, lq, hd], k/v[bh, lk, hd] contiguous; score = scale * <q, k>; causal != 0 hides keys j > i;
 * d_mask (optional float [bh, lq, lk]): entries == 0 set the score to mask_fill (-1e9 for the
 * first-party layer, -inf for a boolean attn_mask).  d_lse[bh, lq] is kept for the backward; d_p
 * (optional [bh, lq, lk]) receives the attention probabilities.  d_scratch: bh*lq floats. */
int rbx_attn_fwd(const float* d_q, const float* d_k, const float* d_v, const float* d_mask, int64_t bh,
                 int32_t lq, int32_t lk, int32_t head_dim, float scale, int32_t causal, float mask_fill,
                 float* d_o, float* d_lse, float* d_p, void* stream);
int rbx_attn_bwd(const float* d_q, const float* d_k, const float* d_v, const float* d_mask, const float* d_o,
                 const float* d_do, const float* d_lse, int64_t bh, int32_t lq, int32_t lk, int32_t head_dim,
                 float scale, int32_t causal, float mask_fill, float* d_dq, float* d_dk, float* d_dv,
                 float* d_scratch, void* stream);

/* The same with DROPOUT ON THE ATTENTION PROBABILITIES, as both reference attentions apply it in training
 * (nn.MultiheadAttention(embed_dim, heads, dropout) inside rechub SASRec, sasrec.py:29,56,81-87 -- default rate 0.5;
 * first-party ScaledDotProductAttention: `attention = self.dropout(attention)`, dot_product_attention.py:40-41):
 * out = (keep o softmax(s) / (1 - p)) V, the normaliser being the undropped sum; d_p, when asked for, receives the
 * dropped probabilities (what the reference returns).  keep(bh, i, j) is a counter-based function of (seed +
 * *d_seed_add, bh, i, j) -- Philox4x32-10, one call per 2 x 4 block of the (query, key) plane, 16-bit decisions,
 * p rounded to a multiple of 2^-16 -- evaluated again by the backward: no mask is stored.  d_seed_add (optional device
 * word): added to `seed` in the kernel, so that a hipGraph replay can draw a new mask (bump it between replays).
 * rbx_attn_dropout_mask writes keep as [bh, lq, lk] bytes (tests; callers that want to inspect the mask).
 * p_drop == 0 is exactly rbx_attn_fwd / rbx_attn_bwd. */
int rbx_attn_dropout_fwd(const float* d_q, const float* d_k, const float* d_v, const float* d_mask, int64_t bh,
                         int32_t lq, int32_t lk, int32_t head_dim, float scale, int32_t causal, float mask_fill,
                         float p_drop, uint64_t seed, const uint64_t* d_seed_add, float* d_o, float* d_lse, float* d_p,
                         void* stream);
int rbx_attn_dropout_bwd(const float* d_q, const float* d_k, const float* d_v, const float* d_mask, const float* d_o,
                         const float* d_do, const float* d_lse, int64_t bh, int32_t lq, int32_t lk, int32_t head_dim,
                         float scale, int32_t causal, float mask_fill, float p_drop, uint64_t seed,
                         const uint64_t* d_seed_add, float* d_dq, float* d_dk, float* d_dv, float* d_scratch,
                         void* stream);
int rbx_attn_dropout_mask(int64_t bh, int32_t lq, int32_t lk, float p_drop, uint64_t seed, const uint64_t* d_seed_add,
                          uint8_t* d_keep, void* stream);

/* The same attention on PACKED operands (MFMA path only: seq_len <= 256, head_dim in {32, 64}, no explicit mask; anything
 * else returns RBX_ERR_UNSUPPORTED): element (b, l, h, d) of a tensor sits at ptr + (b * seq_len + l) * ld + h * head_dim + d.
 * nn.MultiheadAttention projects Q, K, V with Linear layers and then transposes / splits them into [B * H, L, hd] copies
 * (sasrec.py:81-87 through torch/nn/functional.py multi_head_attention_forward); here the kernels read the projections'
 * outputs where they are -- Q [B, L, E], K and V as the two halves of ONE fused [B, L, 2 E] projection (d_k = kv,
 * d_v = kv + E, ldk = ldv = 2 E) -- and write O [B, L, E] for the output projection, dQ, and dK | dV into one
 * [B, L, 2 E] gradient, so no transpose, split or concatenation kernel runs.  d_lse / d_scratch: [batch * heads, seq_len]. */
int rbx_attn_packed_fwd(const float* d_q, int64_t ldq, const float* d_k, int64_t ldk, const float* d_v, int64_t ldv,
                        int64_t batch, int32_t heads, int32_t seq_len, int32_t head_dim, float scale, int32_t causal,
                        float p_drop, uint64_t seed, const uint64_t* d_seed_add, float* d_o, int64_t ldo, float* d_lse,
                        void* stream);
int rbx_attn_packed_bwd(const float* d_q, int64_t ldq, const float* d_k, int64_t ldk, const float* d_v, int64_t ldv,
                        const float* d_o, int64_t ldo, const float* d_do, int64_t lddo, const float* d_lse, int64_t batch,
                        int32_t heads, int32_t seq_len, int32_t head_dim, float scale, int32_t causal, float p_drop,
                        uint64_t seed, const uint64_t* d_seed_add, float* d_dq, int64_t lddq, float* d_dk, int64_t lddk,
                        float* d_dv, int64_t lddv, float* d_scratch, void* stream);

/* ---- K7, second half: the loss epilogue over the sampled logits (one forward pass + fixed-order final sum, one
 * backward pass; ATen runs log_softmax / nll_loss / log_sigmoid / mul / sum and their backward as 4-8 kernels each).
 *   rbx_softmax_ce_*        mean_r [ logsumexp(x[r, :]) - x[r, t_r] ] over logits [rows, n_classes] (row stride in floats):
 *                           core/pytorch/losses/softmax_crossentropy_loss.py:14-22 (t = 0: -log softmax(y_pred)[:, 0]) and
 *                           the CrossEntropyLoss of third_party/rechub/trainers/match_trainer.py:59-60.  d_target NULL = 0;
 *                           a target outside [0, n_classes) sets *d_status (torch raises).  d_lse[rows] is kept for the
 *                           backward, which writes d_dlogits [rows, n_classes] contiguous.
 *   rbx_pair_logsigmoid_*   scale * sum_i -w_i (log sigmoid(pos_i) + log sigmoid(-neg_i)): the pos/neg objective over
 *                           the [B, L] logit blocks of third_party/rechub/models/matching/sasrec.py:100-107 (w = 1 on
 *                           real positions, 0 on padding; NULL = all ones).  A position with w_i == 0 is never evaluated:
 *                           it adds nothing to the loss and rbx_pair_logsigmoid_bwd writes exactly 0 to d_dpos[i] and
 *                           d_dneg[i], whatever pos_i / neg_i hold (inf and NaN included). */
size_t rbx_loss_workspace_size(int64_t n);
int rbx_softmax_ce_fwd(const float* d_logits, int64_t stride, int64_t rows, int32_t n_classes, const int64_t* d_target,
                       float* d_loss, float* d_lse, int32_t* d_status, void* d_workspace, size_t workspace_bytes,
                       void* stream);
int rbx_softmax_ce_bwd(const float* d_logits, int64_t stride, int64_t rows, int32_t n_classes, const int64_t* d_target,
                       const float* d_lse, const float* d_dloss, float* d_dlogits, void* stream);
int rbx_pair_logsigmoid_fwd(const float* d_pos, const float* d_neg, const float* d_weight, int64_t n, float scale,
                            float* d_loss, void* d_workspace, size_t workspace_bytes, void* stream);
int rbx_pair_logsigmoid_bwd(const float* d_pos, const float* d_neg, const float* d_weight, const float* d_dloss, int64_t n,
                            float scale, float* d_dpos, float* d_dneg, void* stream);

/* ---- pooling of a materialised [B,L,D] tensor (standalone pooling modules) ------
 * core/pytorch/layers/sequence.py:4-20, ranking/pytorch/layers/pooling.py:22-40,
 * third_party/rechub/basic/layers.py:176-230.
 * numer_masked: numerator = sum_l mask[b,l]*E[b,l,:] instead of the plain sum.
 * denom: 0 none | 1 #rows whose sum_d != 0 (recbox value mask) | 2 sum_l mask | 3 L.
 * d_inv[B] receives 1/(denom+eps) for the backward. */
int rbx_pool_fwd(const float* d_emb, const float* d_mask, int64_t batch, int32_t seq_len, int32_t dim,
                 int32_t numer_masked, int32_t denom, float eps, float* d_out, float* d_inv, void* stream);
int rbx_pool_bwd(const float* d_dout, const float* d_mask, const float* d_inv, int64_t batch, int32_t seq_len,
                 int32_t dim, int32_t numer_masked, float* d_demb, void* stream);

/* ---- the row-local chains of a SASRec block as single passes over [m, 64] ------------------------------------------
 * third_party/rechub/models/matching/sasrec.py:81-94 (one block of seq_forward) and :110-124 (PointWiseFeedForward).
 * Everything of a block except the attention is local to a row of the [B L, 64] activation; these entry points carry a
 * 32-row slab through the whole chain in registers (csrc/rbx_seqblock.hip) instead of one pass per LayerNorm /
 * projection / residual.  embed_dim is 64 (cfg 5); all activations contiguous with 16-byte aligned bases; biases and
 * LayerNorm parameters may be NULL (0 / 1).
 *   rbx_seqblock_qkv_fwd:  q = LayerNorm(x) (mean, rstd written; q itself only when d_q != NULL); Q = q Wq^T + bq; KV[:, :64] = x Wk^T + bk;
 *                          KV[:, 64:] = x Wv^T + bv, in_w [192, 64] / in_b [192] = nn.MultiheadAttention's in_proj.
 *   rbx_seqblock_ffn_fwd:  with d_attn != NULL first x = res + attn Wo^T + bo (WRITTEN to d_x: `Q + mha_outputs`; with
 *                          d_res_mean / d_res_rstd != NULL d_res is the block input e and res = LayerNorm(e) is rebuilt
 *                          from them and d_res_ln_w / _b, so that rbx_seqblock_qkv_fwd need not store q),
 *                          otherwise d_x is the input; then n = LayerNorm(x) (written to d_n unless NULL),
 *                          h = relu(n W1^T + b1), out = (n + h W2^T + b2) * keep[row] (keep NULL: 1).
 *   rbx_seqblock_ffn_bwd:  the backward of the second chain from its LayerNorm on, one pass: with g = dout * keep[row],
 *                          dW2 = g^T h, db2 = colsum g, dh = (g W2) o [h > 0], dW1 = dh^T n, db1 = colsum dh, dn = dh W1 + g,
 *                          and the LayerNorm backward of dn (dgamma, dbeta, d_dx); n is rebuilt from x, mean, rstd, gamma,
 *                          beta.  Parameter gradients (any may be NULL) are OVERWRITTEN, summed in a fixed order.
 *   rbx_seqblock_attn_in_bwd: behind the attention's backward, one pass: dq = dQ Wq + g (g = the gradient arriving over
 *                          the residual), dgamma / dbeta and the LayerNorm backward of dq, de = that + dK Wk + dV Wv
 *                          (d_dKV [m, 128] = dK | dV), stored as de * row_scale[row] * alpha when d_row_scale != NULL (the backward of SASRec's
 *                          input stage `(alpha e + position) * keep`, sasrec.py:68-77, folded into the first block).  The
 *                          three in-projection weight gradients are not part of it. */
/*   rbx_seqblock_inproj_dw: the three in-projection weight gradients in one pass: d_dw [192, 64] = dQ^T q | dK^T x | dV^T x
 *                          (nn.MultiheadAttention.in_proj_weight's layout), d_db [192] = their column sums; q = LayerNorm(x)
 *                          is rebuilt from x, mean, rstd, gamma, beta.  Either output may be NULL.
 *   rbx_seqblock_attn_out_bwd: the out-projection's backward, one pass: dO = g Wo, dWo = g^T O, dbo = colsum g. */
int rbx_seqblock_qkv_fwd(const float* d_x, int64_t m, const float* d_ln_w, const float* d_ln_b, float eps,
                         const float* d_in_w, const float* d_in_b, float* d_mean, float* d_rstd, float* d_q, float* d_Q,
                         float* d_KV, void* stream);
int rbx_seqblock_ffn_fwd(const float* d_attn, const float* d_res, const float* d_wo, const float* d_bo, float* d_x, int64_t m,
                         const float* d_ln_w, const float* d_ln_b, float eps, const float* d_w1, const float* d_b1,
                         const float* d_w2, const float* d_b2, const float* d_keep, float* d_mean, float* d_rstd, float* d_n,
                         float* d_h, float* d_out, const float* d_res_mean, const float* d_res_rstd, const float* d_res_ln_w,
                         const float* d_res_ln_b, void* stream);
size_t rbx_seqblock_ffn_bwd_workspace_size(int64_t m);
int rbx_seqblock_ffn_bwd(const float* d_dout, const float* d_keep, const float* d_h, const float* d_x, const float* d_mean,
                         const float* d_rstd, int64_t m, const float* d_ln_w, const float* d_ln_b, const float* d_w1,
                         const float* d_w2, float* d_dx, float* d_dw1, float* d_db1, float* d_dw2, float* d_db2,
                         float* d_dgamma, float* d_dbeta, void* d_workspace, size_t workspace_bytes, void* stream);
size_t rbx_seqblock_attn_in_bwd_workspace_size(int64_t m);
int rbx_seqblock_attn_in_bwd(const float* d_dQ, const float* d_dKV, const float* d_g, const float* d_x, const float* d_mean,
                             const float* d_rstd, int64_t m, const float* d_ln_w, const float* d_in_w,
                             const float* d_row_scale, float alpha, float* d_de, float* d_dgamma, float* d_dbeta,
                             void* d_workspace, size_t workspace_bytes, void* stream);
size_t rbx_seqblock_attn_out_bwd_workspace_size(int64_t m);
int rbx_seqblock_attn_out_bwd(const float* d_g, const float* d_O, int64_t m, const float* d_wo, float* d_dO, float* d_dwo,
                              float* d_dbo, void* d_workspace, size_t workspace_bytes, void* stream);
size_t rbx_seqblock_inproj_dw_workspace_size(int64_t m);
int rbx_seqblock_inproj_dw(const float* d_dQ, const float* d_dKV, const float* d_x, const float* d_mean, const float* d_rstd,
                           int64_t m, const float* d_ln_w, const float* d_ln_b, float* d_dw, float* d_db, void* d_workspace,
                           size_t workspace_bytes, void* stream);

/* ---- DIN's local activation unit (rbx_din.hip) ---------------------------------------------------------------------------
 * d_hist [batch, seq_len, dim]: the rows of a sample contiguous, samples hist_stride_b floats apart; d_target [batch, dim]
 * at a row stride of target_stride_b (a slice of a wider block is read in place).  Everything written is contiguous.
 *   rbx_din_pairs_fwd   d_y [batch * seq_len, n] = act([t, h, t - h, t o h] W^T + bias), d_w [n, 4 dim] with the four column
 *                       blocks in that order, act 0 | 1 = ReLU, d_bias may be NULL.  The [batch * seq_len, 4 dim] operand is
 *                       never stored: it is formed from h and t on the way into the fp32 matrix cores.
 *   rbx_din_pairs_bwd   with dP = dy' W (dy' = d_dy where d_y > 0 when act = 1; d_y may be NULL when act = 0), never stored:
 *                       d_dhist [batch, seq_len, dim] = dP_b - dP_c + dP_d o t, d_dtarget [batch, dim] = sum_l (dP_a + dP_c
 *                       + dP_d o h), d_dw [n, 4 dim] = dy'^T [t, h, t - h, t o h], d_db [n] = column sums of dy'.  Each of
 *                       the four may be NULL; the workspace is needed for d_dw / d_db.  All sums run in a fixed order.
 *   rbx_din_pool_fwd    d_weight [batch, seq_len] = score o mask, or with softmax != 0 softmax over seq_len of
 *                       score o mask + (-1e9)(1 - mask) (a fully masked sample gets 1 / seq_len); d_mask may be NULL (no mask
 *                       terms).  d_out [batch, dim] = sum_l weight[b, l] h[b, l, :].  d_score, d_mask, d_weight contiguous.
 *   rbx_din_pool_bwd    d_dscore [batch, seq_len] = (softmax ? w o (dw - sum_l w dw) : dw) o mask with dw[l] = <dout, h_l>;
 *                       d_dhist [batch, seq_len, dim] = w_l dout.  Either may be NULL.
 * Supported: dim a multiple of 4 in [4, 128]; 1 <= n <= 64; batch * seq_len <= INT_MAX; the pool calls seq_len <= 4096;
 * 16-byte aligned bases (d_hist, d_target, d_w, d_dhist), strides multiples of 4.  Anything else: RBX_ERR_UNSUPPORTED before
 * any launch.  batch = 0 launches nothing.  No call allocates or reads back: all are capturable. */
int rbx_din_pairs_fwd(const float* d_hist, int64_t hist_stride_b, const float* d_target, int64_t target_stride_b,
                      int64_t batch, int32_t seq_len, int32_t dim, const float* d_w, const float* d_bias, int32_t n,
                      int32_t act, float* d_y, void* stream);
size_t rbx_din_pairs_bwd_workspace_size(int64_t batch, int32_t seq_len, int32_t dim, int32_t n);
int rbx_din_pairs_bwd(const float* d_hist, int64_t hist_stride_b, const float* d_target, int64_t target_stride_b,
                      int64_t batch, int32_t seq_len, int32_t dim, const float* d_w, int32_t n, int32_t act,
                      const float* d_y, const float* d_dy, float* d_dhist, float* d_dtarget, float* d_dw, float* d_db,
                      void* d_workspace, size_t workspace_bytes, void* stream);
int rbx_din_pool_fwd(const float* d_score, const float* d_mask, const float* d_hist, int64_t hist_stride_b, int64_t batch,
                     int32_t seq_len, int32_t dim, int32_t softmax, float* d_weight, float* d_out, void* stream);
int rbx_din_pool_bwd(const float* d_dout, const float* d_weight, const float* d_mask, const float* d_hist,
                     int64_t hist_stride_b, int64_t batch, int32_t seq_len, int32_t dim, int32_t softmax, float* d_dscore,
                     float* d_dhist, void* stream);

/* ---- field-aware FM: gather and cross, no [B, F, F, D] tensor (csrc/rbx_ffm.hip; additions only, the version stays) ----
 * Replaces third_party/rechub/models/ranking/deepffm.py:58-66 / :133-141 (the ffm_embedding lookups of x * F +
 * fields_offset, concatenated to [B, F, F, D]) together with basic/layers.py:651-680 (FFM: P = F(F-1)/2 sliced
 * multiplies and a stack) and their autograd backward.  F = n_fields one-id categorical descriptors (pool NONE, seq_len 1)
 * of one dim D; fields[i].table is the contiguous [vocab_i, D] weight of the reference's nn.Embedding, an id x of field i
 * names its rows x*F .. x*F+F-1.  With E[b,i,j] = table_i[x_i(b)*F + j] and the pairs i < j in the reference's order (i
 * outer, j inner):
 *   reduce_sum == 0   d_out[b * out_stride_b + p(i,j) * D + d] = E[b,i,j][d] * E[b,j,i][d]        ([B, P, D])
 *   reduce_sum != 0   d_out[b * out_stride_b + p(i,j)]         = sum_d of that product            ([B, P])
 * Ids are read in place (any rbx_dtype_t, element stride ids_stride_b) as rbx_embed_fwd reads them.  The diagonal rows
 * E[b,i,i] are never read.  An id with x < 0 or x*F + F > vocab_i reads as a block of zeros and sets bit 0 of *d_status.
 *   rbx_ffm_fwd    one launch; reads F(F-1) rows and writes P rows (or P floats) per sample.
 *   rbx_ffm_sort   the (block, sample) pairs of every field with a gradient, sorted by the passes of rbx_embed_sort over
 *                  the view of table i as [vocab_i / F, F*D].  fields[i].grad: non-NULL for every table that will get a
 *                  gradient (the pointer is not used here: a placeholder does), as in the rbx_ffm_bwd that follows.
 *   rbx_ffm_bwd    dense [vocab_i, D] gradients into fields[i].grad (NULL = frozen): dE[b,i,j] = dout[b, p(i,j)] o E[b,j,i]
 *                  is formed inside the segmented reduce and never stored; the partner ids are read in place.  Every touched
 *                  block is written once -- its diagonal row i with zeros --; accumulate as in rbx_embed_bwd (0: the caller
 *                  zero-filled the gradients, touched blocks are stored; else read-modify-write).  No float atomics: the
 *                  same bits from run to run.  The workspace is that of rbx_ffm_sort for the same fields and batch.
 * RBX_ERR_UNSUPPORTED before anything is launched or cleared: D % 4 != 0 or D > 128; F < 2 or F > RBX_MAX_FIELDS;
 * F * D > 1024; a table_stride other than dim; a padding_idx; two descriptors with one table; a table, gradient or (with
 * reduce_sum == 0) d_out / d_dout base that is not 16-byte aligned, or a row stride of those that is not a multiple of 4.
 * A vocab below F (no whole block) is RBX_ERR_INVALID.  batch == 0: RBX_OK, nothing launched.  All calls are capturable. */
int rbx_ffm_fwd(const rbx_field_t* fields, int32_t n_fields, int64_t batch, int32_t reduce_sum, float* d_out,
                int64_t out_stride_b, int32_t* d_status, void* stream);
size_t rbx_ffm_bwd_workspace_size(const rbx_field_t* fields, int32_t n_fields, int64_t batch);
int rbx_ffm_sort(const rbx_field_t* fields, int32_t n_fields, int64_t batch, void* d_workspace, size_t workspace_bytes,
                 int32_t* d_status, void* stream);
int rbx_ffm_bwd(const rbx_field_t* fields, int32_t n_fields, int64_t batch, int32_t reduce_sum, const float* d_dout,
                int64_t dout_stride_b, int32_t accumulate, void* d_workspace, size_t workspace_bytes, void* stream);

/* ---- multi-interest dynamic routing: MIND, ComirecDR (csrc/rbx_capsule.hip; additions only, the version stays) -----------
 * Replaces third_party/rechub/basic/layers.py:588-643 (CapsuleNetwork.forward) and its autograd backward.  B = batch,
 * L = seq_len, D = dim, K = interests, N = K D.  hat is addressed as hat[b sb + k sk + l sl + e]: [B, L, N] with sk = D for
 * the per-interest forms, [B, L, D] with sk = 0 for the shared form (bilinear_type 0, layers.py:590-591).
 *   rbx_capsule_hat          layers.py:595-596, whose product is [B, L, N, D]: d_hat [B, L, N] (contiguous) with
 *                            hat[b, l, n] = sum_d w[l, n, d] x[b, l, d], one fp32-MFMA GEMM per position; d_x is read in place at
 *                            x[b x_stride_b + l x_stride_l + d], d_w is the contiguous [L, N, D] parameter.
 *   rbx_capsule_route_fwd    layers.py:607-641 for one (b, k) per wavefront with its [L, D] slice of hat in LDS: `updates`
 *                            (0..2 = min(routing_times - 1, 2)) rounds of c = softmax_l(logits) set to 0 where the mask is 0
 *                            (not renormalised), s = sum_l c[l] hat[l], v = squash(s), logits += hat v, then the output round.
 *                            d_init [B, K, L]: the starting logits, NULL = zeros.  The mask is read in place at
 *                            mask[b mask_stride_b + l mask_stride_l] as RBX_I32 / RBX_I64 / RBX_F32 / RBX_MASK_U8 (bool).
 *                            Writes d_v [B, K, D], and what the backward needs: d_c [B, K, L], d_s [B, K, D].  No atomics.
 *   rbx_capsule_route_bwd    the output round's gradient (earlier rounds are detached, layers.py:602-603): d_ds [B, K, D] =
 *                            f(n) dv + 2 f'(n) (s . dv) s with n = |s|^2, f(n) = n / (1 + n) / sqrt(n + 1e-9) (NULL: not stored);
 *                            d_dhat (NULL: not formed) = c ds in hat's layout: [B, L, N], or with shared != 0 [B, L, D] summed
 *                            over k in order.
 *   rbx_capsule_bilinear_dx  d_dx [B, L, D] = sum_n G[b, l, n] w[l, n, d]
 *   rbx_capsule_bilinear_dw  d_dw [L, N, D] = sum_b G[b, l, n] x[b, l, d]; samples are summed in splits of
 *                            rbx_capsule_dw_split() whose partial sums (in the workspace) are added in order.
 *                            G[b, l, n] = g[b g_stride_b + l g_stride_l + n], times c[b, n / D, l] when d_c is given: with
 *                            g = ds (g_stride_b = N, g_stride_l = 0) the operand c ds is formed on the way into the MFMA and
 *                            neither d_hat nor a [B, L, N, D] tensor exists; with g = a stored d_hat and d_c = NULL they are the
 *                            backward of rbx_capsule_hat alone.
 * Supported: D a multiple of 4 in [4, 128]; 1 <= K <= 32; L (D + 1) + 3 L + D <= 14336 floats for the routing call
 * (rbx_capsule_route_supported; covers L = 200 at D = 64 and L = 50 at D = 128); 16-byte aligned float bases and strides that
 * are multiples of 4.  Anything else: RBX_ERR_UNSUPPORTED before any launch.  batch = 0 launches nothing (dw: zeros).  No
 * call allocates or reads back: all are capturable. */
#define RBX_MASK_U8 4
int rbx_capsule_route_supported(int32_t seq_len, int32_t dim);
int32_t rbx_capsule_dw_split(void);
int rbx_capsule_hat(const float* d_x, int64_t x_stride_b, int64_t x_stride_l, const float* d_w, int64_t batch,
                    int32_t seq_len, int32_t dim, int32_t interests, float* d_hat, void* stream);
int rbx_capsule_route_fwd(const float* d_hat, int64_t hat_stride_b, int64_t hat_stride_k, int64_t hat_stride_l,
                          const void* d_mask, int32_t mask_dtype, int64_t mask_stride_b, int64_t mask_stride_l,
                          const float* d_init, int64_t batch, int32_t interests, int32_t seq_len, int32_t dim,
                          int32_t updates, float* d_v, float* d_c, float* d_s, void* stream);
int rbx_capsule_route_bwd(const float* d_dv, const float* d_s, const float* d_c, int64_t batch, int32_t interests,
                          int32_t seq_len, int32_t dim, int32_t shared, float* d_ds, float* d_dhat, void* stream);
int rbx_capsule_bilinear_dx(const float* d_w, const float* d_g, int64_t g_stride_b, int64_t g_stride_l, const float* d_c,
                            int64_t batch, int32_t seq_len, int32_t dim, int32_t interests, float* d_dx, void* stream);
size_t rbx_capsule_bilinear_dw_workspace_size(int64_t batch, int32_t seq_len, int32_t dim, int32_t interests);
int rbx_capsule_bilinear_dw(const float* d_x, int64_t x_stride_b, int64_t x_stride_l, const float* d_g, int64_t g_stride_b,
                            int64_t g_stride_l, const float* d_c, int64_t batch, int32_t seq_len, int32_t dim,
                            int32_t interests, float* d_dw, void* d_workspace, size_t workspace_bytes, void* stream);

/* ---- GRU recurrence: GRU4Rec, NARM (csrc/rbx_gru.hip; additions only, the version stays) ----------------------------------
 * Replaces torch.nn.GRU under third_party/rechub/models/matching/gru4rec.py:40-44, 66-67 and narm.py:30, 50-55 (there with
 * pack_padded_sequence / pad_packed_sequence around it, whose lengths narm.py:49 copies to the host).  B = batch, L = seq_len,
 * H = hidden.  torch's gate convention: rows of d_w_hh [3H, H] (contiguous) and d_b_hh [3H] (NULL: none) are ordered r, z, n;
 *   gh = h W_hh^T + b_hh   r = s(gi_r + gh_r)   z = s(gi_z + gh_z)   n = tanh(gi_n + r gh_n)   h' = (1 - z) n + z h.
 * gi = x W_ih^T + b_ih comes from rbx_linear_fwd and is read at gi[b gi_stride_b + t gi_stride_t + c], c < 3H.
 *   rbx_gru_fwd   one launch for all L steps: a workgroup owns 16 samples, gh runs on v_mfma_f32_16x16x4_f32 against W_hh held
 *                 in registers, h stays on chip.  d_h0 [B, H] (NULL: zeros).  d_lengths [B] (RBX_I32 / RBX_I64; NULL: all L),
 *                 clamped to [0, L]: for t >= lengths[b] the state is frozen and d_out[b, t, :] = 0; d_hn[b] is the state after
 *                 step lengths[b] - 1 (length 0: h0).  Writes d_out [B, L, H], d_hn [B, H] and, for the backward,
 *                 d_saved [B, L, 5, H] = r, z, n, gh_n, h_prev of every position (h_prev is also the x operand of dW_hh).
 *   rbx_gru_bwd   one launch, t = L-1 .. 0 with dh on chip.  d_dout (NULL: none) is read at
 *                 dout[b dout_stride_b + t dout_stride_t + j]; d_dhn [B, H] (NULL: none).  Writes d_dgi [B, L, 3H] (the
 *                 gradient of gi), d_dghn [B, L, H] = d_gi_n r (the n-gate columns in which the gradient of gh differs from
 *                 d_dgi) and d_dh0 [B, H]; positions at and beyond a sample's length get zeros.
 * dW_ih, dx, dW_hh and the bias gradients are rbx_linear_bwd calls over these matrices.
 * Supported (rbx_gru_supported): H a multiple of 4 in [4, 128], L >= 1; dtype (the RBX_* code of every float tensor) must be
 * RBX_F32; gi and d_dout 16-byte aligned with strides that are multiples of 4.  Anything else: RBX_ERR_UNSUPPORTED before any
 * launch.  batch = 0 launches nothing.  No atomics, sums in a fixed order; no call allocates or reads back: capturable. */
int rbx_gru_supported(int32_t hidden, int32_t seq_len);
int rbx_gru_fwd(const float* d_gi, int64_t gi_stride_b, int64_t gi_stride_t, const float* d_w_hh, const float* d_b_hh,
                const float* d_h0, const void* d_lengths, int32_t lengths_dtype, int64_t batch, int32_t seq_len,
                int32_t hidden, int32_t dtype, float* d_out, float* d_saved, float* d_hn, void* stream);
int rbx_gru_bwd(const float* d_saved, const float* d_w_hh, const float* d_dout, int64_t dout_stride_b, int64_t dout_stride_t,
                const float* d_dhn, const void* d_lengths, int32_t lengths_dtype, int64_t batch, int32_t seq_len,
                int32_t hidden, int32_t dtype, float* d_dgi, float* d_dghn, float* d_dh0, void* stream);

/* ---- attention-gated GRU recurrence: DIEN's AGRU / AUGRU (csrc/rbx_gru.hip; additions only, the version stays) ----------
 * Replaces DynamicRNN over AGRUCell / AUGRUCell of third_party/recbole/model/sequential_recommender/dien.py:389-521 (a Python
 * loop over the steps of a PackedSequence, whose lengths dien.py:336 copies to the host).  B = batch, L = seq_len, H = hidden.
 * The reference's gate convention: rows of d_w_hh [3H, H] (contiguous) and d_b_hh [3H] (NULL: none) are ordered r, u, n (its
 * chunk(3, 1); torch's r, z, n); a = d_att[b L + t], d_att [B, L] contiguous, taken as written (no clamp);
 *   gh = h W_hh^T + b_hh   r = s(gi_r + gh_r)   u = s(gi_u + gh_u)   n = tanh(gi_n + r gh_n)
 *   cell 1 (AUGRU): c = a u     cell 0 (AGRU): c = a (u is not formed)     h' = (1 - c) h + c n.
 * gi = x W_ih^T + b_ih comes from rbx_linear_fwd and is read at gi[b gi_stride_b + t gi_stride_t + c], c < 3H.
 *   rbx_attgru_fwd   one launch for all L steps: a workgroup owns 16 samples, gh runs on v_mfma_f32_16x16x4_f32 against W_hh
 *                    held in registers, h stays on chip.  d_h0 [B, H] (NULL: zeros).  d_lengths [B] (RBX_I32 / RBX_I64; NULL: all
 *                    L), clamped to [0, L]: for t >= lengths[b] the state is frozen and d_out[b, t, :] = 0; d_hn[b] is the state
 *                    after step lengths[b] - 1 (length 0: h0).  Writes d_out [B, L, H], d_hn [B, H] and, for the backward,
 *                    d_saved [B, L, 5, H] = r, u, n, gh_n, h_prev of every position (h_prev is also the x operand of dW_hh;
 *                    cell 0 leaves the u slot unwritten).
 *   rbx_attgru_bwd   one launch, t = L-1 .. 0 with dh on chip.  d_dout (NULL: none) is read at
 *                    dout[b dout_stride_b + t dout_stride_t + j]; d_dhn [B, H] (NULL: none).  Writes d_dgi [B, L, 3H] (the
 *                    gradient of gi; cell 0: zeros in the u columns), d_dghn [B, L, H] = d_gi_n r (the n-gate columns in which
 *                    the gradient of gh differs from d_dgi), d_datt [B, L] (the gradient of the score: a sum over the hidden
 *                    units, in a fixed order) and d_dh0 [B, H]; positions at and beyond a sample's length get zeros.
 * dW_ih, dx, dW_hh and the bias gradients are rbx_linear_bwd calls over these matrices.
 * Supported (rbx_attgru_supported): H a multiple of 4 in [4, 128], L >= 1, cell 0 or 1; dtype (the RBX_* code of every float
 * tensor) must be RBX_F32; gi and d_dout 16-byte aligned with strides that are multiples of 4.  Anything else:
 * RBX_ERR_UNSUPPORTED before any launch.  batch = 0 launches nothing.  No atomics, sums in a fixed order; no call allocates or
 * reads back: capturable. */
int rbx_attgru_supported(int32_t hidden, int32_t seq_len, int32_t cell);
int rbx_attgru_fwd(const float* d_gi, int64_t gi_stride_b, int64_t gi_stride_t, const float* d_att, const float* d_w_hh,
                   const float* d_b_hh, const float* d_h0, const void* d_lengths, int32_t lengths_dtype, int64_t batch,
                   int32_t seq_len, int32_t hidden, int32_t cell, int32_t dtype, float* d_out, float* d_saved, float* d_hn,
                   void* stream);
int rbx_attgru_bwd(const float* d_saved, const float* d_att, const float* d_w_hh, const float* d_dout, int64_t dout_stride_b,
                   int64_t dout_stride_t, const float* d_dhn, const void* d_lengths, int32_t lengths_dtype, int64_t batch,
                   int32_t seq_len, int32_t hidden, int32_t cell, int32_t dtype, float* d_dgi, float* d_dghn, float* d_datt,
                   float* d_dh0, void* stream);

/* ---- expert-gate mixing: MMOE, CGC / PLE, AITM (csrc/rbx_mix.hip; additions only, the version stays) -----------------------
 * Replaces, under third_party/rechub/models/multi_task/mmoe.py:46-57, ple.py:102-128 and aitm.py:77-84, the torch.cat of the
 * expert outputs into [B, E, H], one torch.mul per gate into another [B, E, H], and a torch.sum.  B = batch, H = hidden,
 * E = experts, T = gates.  Gate t mixes the experts sel[sel_off[t]] .. sel[sel_off[t + 1] - 1] (n_t of them, distinct):
 *   p_t[b, j] = softmax_j(z_t[b, j]) (softmax != 0; max-subtracted, fp32) or z_t[b, j];  out_t[b, :] = sum_j p_t[b, j] X_sel_t[j][b, :]
 * x [E], x_stride [E], z [T], sel, sel_off [T + 1], dout [T], dx [E], dz [T] are HOST arrays; what x, z, dout, dx, dz hold are
 * device pointers.  Expert e is read at x[e][b x_stride[e] + c], c < H; z[t] is a contiguous [B, n_t].  Everything travels to
 * the kernel by value in its argument struct: a call is ONE kernel launch on `stream` and nothing else -- no allocation, copy,
 * memset, stream, event, synchronisation, device-side table or workspace: capturable.
 *   rbx_expert_mix_fwd  one pass over the experts for all T gates (X_e[b, :] is loaded once, whichever gates select e).  Writes
 *                       d_out [T, B, H] and, with softmax, d_p [B, sel_off[T]] (gate t in columns sel_off[t] ..) for the backward
 *                       (without softmax d_p is not written and may be NULL).
 *   rbx_expert_mix_bwd  one pass again.  dout[t] [B, H] contiguous (NULL: that output had no gradient = zeros).  Writes, where
 *                       the pointer is not NULL (dx or dz themselves may be NULL), dx[e] [B, H] = sum over (t, j) with
 *                       sel_t[j] = e of p_t[b, j] dout_t[b, :] in full (zeros if no gate selects e) and dz[t] [B, n_t]:
 *                       dp_t[b, j] = <dout_t[b, :], X_sel_t[j][b, :]>, dz = p (dp - sum_i p_i dp_i) with softmax (d_p as the
 *                       forward wrote it; z is not read), else dp (z is read as p).
 * Supported (rbx_expert_mix_supported): dtype (the RBX_* code of every float tensor) RBX_F32; H a multiple of 4 in [4, 1024];
 * 1 <= E <= 16; 1 <= T <= 8; 1 <= n_t <= 16, every entry of sel in [0, E) and no expert twice in one gate; x, d_out, dout and
 * dx 16-byte aligned, x_stride multiples of 4.  Anything else: RBX_ERR_UNSUPPORTED before any launch.  batch = 0 launches
 * nothing.  No atomics, sums in a fixed order (out_t in ascending expert order, dx in ascending gate order). */
int rbx_expert_mix_supported(int32_t hidden, int32_t experts, int32_t gates, const int32_t* sel, const int32_t* sel_off,
                             int32_t dtype);
int rbx_expert_mix_fwd(const float* const* x, const int64_t* x_stride, const float* const* z, const int32_t* sel,
                       const int32_t* sel_off, int64_t batch, int32_t hidden, int32_t experts, int32_t gates, int32_t softmax,
                       int32_t dtype, float* d_out, float* d_p, void* stream);
int rbx_expert_mix_bwd(const float* const* x, const int64_t* x_stride, const float* const* z, const float* d_p,
                       const float* const* dout, const int32_t* sel, const int32_t* sel_off, int64_t batch, int32_t hidden,
                       int32_t experts, int32_t gates, int32_t softmax, int32_t dtype, float* const* dx, float* const* dz,
                       void* stream);

/* ---- additive attention pooling: NARM, STAMP (csrc/rbx_addattn.hip; additions only, the version stays) ---------------------
 * Replaces the ATen lines third_party/rechub/models/matching/narm.py:60-68 (Eq. 6-8) and stamp.py:69-72 (Eq. 7-8), whose
 * x W^T [B, L, H] is written, re-read three times and kept by autograd.  B = batch, L = seq_len, D = dim, H = hidden:
 *   q[b,l] = v . sigmoid(x[b,l] W^T + ctx[b])      e[b,l] = exp(q[b,l]) mask[b,l]   (as written: no max subtraction)
 *   alpha[b,l] = e[b,l] / max(sum_l e[b,l], eps)    out[b] = sum_l alpha[b,l] x[b,l]
 * d_x is read at x[b x_stride_b + l x_stride_l + c], c < D; d_w [H, D] contiguous; d_ctx [B, H] (NULL: zeros); d_v [H];
 * d_mask [B, L] contiguous as RBX_I32 / RBX_I64 / RBX_F32 / RBX_MASK_U8 (bool), nonzero = valid (NULL: all valid).
 *   rbx_addattn_fwd  one launch.  x W^T runs tile by tile (16 positions) on v_mfma_f32_16x16x4_f32 against W held in
 *                    registers for all samples of a workgroup; sigmoid, the v product, exp, the mask and the sums stay on
 *                    chip.  The division is an IEEE division: one valid position gives alpha = 1 exactly, k equal logits
 *                    1.0f / k.  eps = 0 and no valid position: NaN, as the composition; eps > 0: alpha = 0, out = 0.
 *                    Writes d_out [B, D] and d_alpha [B, L].
 *   rbx_addattn_bwd  d_dout is read at dout[b dout_stride_b + c]; alpha has no gradient of its own.  One launch recomputes
 *                    s = sigmoid(x W^T + ctx) per tile and forms g_l = dout . x_l, dq_l = alpha_l (g_l - sum_j alpha_j g_j),
 *                    dpre_lh = dq_l v_h s_lh (1 - s_lh); writes d_dctx [B, H] = sum_l dpre_l, d_dx [B, L, D] =
 *                    alpha_l dout + dpre_l W, and d_dpre [B, L, H] (NULL: not wanted) -- a transient of the backward from
 *                    which rbx_linear_bwd forms dW = dpre^T x.  dv = sum_{b,l} dq_l s_l: one row of H floats per workgroup in
 *                    the workspace (rbx_addattn_bwd_workspace_size), summed in a fixed order by a second launch into d_dv [H].
 * Supported (rbx_addattn_supported): D and H multiples of 4 in [4, 128], L >= 1; dtype (the RBX_* code of every float tensor)
 * RBX_F32; x and d_dout 16-byte aligned with strides that are multiples of 4.  Anything else: RBX_ERR_UNSUPPORTED before any
 * launch.  batch = 0 launches nothing.  No atomics, sums in a fixed order; no call allocates or reads back: capturable. */
int rbx_addattn_supported(int32_t dim, int32_t hidden, int32_t seq_len);
int rbx_addattn_fwd(const float* d_x, int64_t x_stride_b, int64_t x_stride_l, const float* d_w, const float* d_ctx,
                    const float* d_v, const void* d_mask, int32_t mask_dtype, float eps, int64_t batch, int32_t seq_len,
                    int32_t dim, int32_t hidden, int32_t dtype, float* d_out, float* d_alpha, void* stream);
size_t rbx_addattn_bwd_workspace_size(int64_t batch, int32_t hidden);
int rbx_addattn_bwd(const float* d_dout, int64_t dout_stride_b, const float* d_x, int64_t x_stride_b, int64_t x_stride_l,
                    const float* d_w, const float* d_ctx, const float* d_v, const void* d_mask, int32_t mask_dtype,
                    const float* d_alpha, float eps, int64_t batch, int32_t seq_len, int32_t dim, int32_t hidden,
                    int32_t dtype, float* d_dx, float* d_dctx, float* d_dv, float* d_dpre, void* d_workspace,
                    size_t workspace_bytes, void* stream);

/* ---- Attentional FM: pair-attention pooling (csrc/rbx_afm.hip; additions only, the version stays) ---------------------------
 * Replaces the ATen lines of RecBole's AFM (third_party/recbole/model/context_aware_recommender/afm.py:75-99 over AttLayer,
 * model/layers.py:236-261), whose pair products [B, P, D] and attention hidden layer [B, P, A] are written and kept by
 * autograd.  B = batch, F = n_fields, D = dim, A = att_dim, P = F (F - 1) / 2 pairs k = (i, j), i < j, in row-major order:
 *   p_k = x_i * x_j      s_k = sum_a h_a relu(W p_k)_a      a = softmax_k(s)      out = sum_k a_k p_k
 * d_x is read at x[b x_stride_b + f x_stride_f + c], c < D; d_w [A, D] contiguous (no bias); d_h [A].
 *   rbx_afm_fwd  one launch.  A wavefront stages one sample's x [F, D] in LDS and walks its pairs in tiles of 16: W p_k runs
 *                on v_mfma_f32_16x16x4_f32 (A and the last tile padded inside the kernel) with p_k formed on the fly; relu,
 *                the h product, the max-subtracted softmax and the weighted sum stay on chip.  The division is an IEEE
 *                division: one pair gives a = 1 exactly, P equal logits 1.0f / P.  Writes d_out [B, D], d_stat [2, B] (the
 *                maximum logit, then the sum of exp(s - max), per sample) and, when not NULL, d_attn [B, P].
 *   rbx_afm_bwd  d_dout is read at dout[b dout_stride_b + c]; d_out and d_stat as the forward wrote them; attn has no
 *                gradient of its own.  One launch recomputes p_k, the pre-activations and a_k and forms ds_k = a_k (dout . p_k
 *                - dout . out), dpre_k = ds_k h [pre_k > 0], dp_k = a_k dout + W^T dpre_k; dx_i += dp_k x_j and dx_j +=
 *                dp_k x_i are added on chip and d_dx [B, F, D] is written once.  dW = sum dpre_k p_k^T and dh = sum ds_k
 *                relu(pre_k): one row of A D + A floats per wavefront in the workspace (rbx_afm_bwd_workspace_size), summed
 *                in a fixed order by a second launch into d_dw [A, D] and d_dh [A].  d_dx, d_dw, d_dh: NULL skips it.
 * Supported (rbx_afm_supported): 2 <= F <= 39; D a multiple of 4 in [4, 64]; 1 <= A <= 64; dtype (the RBX_* code of every float
 * tensor) RBX_F32; x and d_dout 16-byte aligned with strides that are multiples of 4.  Anything else: RBX_ERR_UNSUPPORTED
 * before any launch.  batch = 0 launches nothing.  No atomics, sums in a fixed order; no call allocates or reads back:
 * capturable. */
int rbx_afm_supported(int32_t n_fields, int32_t dim, int32_t att_dim);
int rbx_afm_fwd(const float* d_x, int64_t x_stride_b, int64_t x_stride_f, const float* d_w, const float* d_h, int64_t batch,
                int32_t n_fields, int32_t dim, int32_t att_dim, int32_t dtype, float* d_out, float* d_stat, float* d_attn,
                void* stream);
size_t rbx_afm_bwd_workspace_size(int64_t batch, int32_t n_fields, int32_t dim, int32_t att_dim);
int rbx_afm_bwd(const float* d_dout, int64_t dout_stride_b, const float* d_x, int64_t x_stride_b, int64_t x_stride_f,
                const float* d_w, const float* d_h, const float* d_out, const float* d_stat, int64_t batch, int32_t n_fields,
                int32_t dim, int32_t att_dim, int32_t dtype, float* d_dx, float* d_dw, float* d_dh, void* d_workspace,
                size_t workspace_bytes, void* stream);

/* ---- AutoInt: multi-head self-attention over the fields, one layer (csrc/rbx_fieldattn.hip; additions only, the version stays)
 * Replaces, per layer of third_party/recbole/model/context_aware_recommender/autoint.py:88-98, nn.MultiheadAttention called as
 * attn(x, x, x) on the [F, B, E] view: the in-projection into [F, B, 3 E], three head-major copies, the [B h, F, F] scores
 * written, soft-maxed, dropped out and re-read, their average over the heads and the out-projection.  B = batch, F = n_fields,
 * E = dim, h = heads, dh = E / h.  Per sample, x [F, E]:
 *   q | k | v = x Win^T + bin       S_t = (q_t dh^-1/2) k_t^T       P_t = softmax over the keys (max-subtracted)
 *   P~_t = keep_t * P_t * 65536 / (65536 - thr16)   (p_drop > 0)       o = concat_t P~_t v_t
 *   z = o Wout^T + bout             y = z [+ res] [then relu]
 * d_x is read at x[b x_stride_b + f x_stride_f + e], so the reference's [F, B, E] view and a [B, F, E] tensor both come in
 * without a copy; d_res (NULL: none) likewise.  d_in_w [3 E, E], d_in_b [3 E] or NULL, d_out_w [E, E], d_out_b [E] or NULL,
 * contiguous.  keep(b h + t, query, key) is the function of rbx_attn_dropout_fwd with the same (p_drop, seed, d_seed_add):
 * rbx_attn_dropout_mask(B h, F, F, ...) returns the mask these kernels use; nothing is stored, p_drop = 0 draws nothing.
 *   rbx_fieldattn_fwd  one launch.  A wavefront stages one sample's x in LDS (field rows padded to 16 inside the kernel); both
 *                      projections, q k^T and P v run on v_mfma_f32_16x16x4_f32; q, k, v, the probabilities and o stay on
 *                      chip.  Writes d_y [B, F, E] and, when not NULL, the pre-dropout probabilities d_attn [B, h, F, F].
 *   rbx_fieldattn_bwd  d_dy is read at dy[b dy_stride_b + f dy_stride_f + e]; d_y (the forward's, needed only with relu) gives
 *                      the relu mask.  One launch recomputes q, k, v, P, the mask and o with the forward's instructions and
 *                      writes d_dx [B, F, E] and d_dres [B, F, E] (= dy under the relu mask); the weight and bias gradients
 *                      are summed per wavefront into one workspace row of 4 E E + 4 E floats
 *                      (rbx_fieldattn_bwd_workspace_size: at most 2048 rows, whatever the batch) and a second launch adds the
 *                      rows in a fixed order into d_din_w [3 E, E], d_din_b [3 E], d_dout_w [E, E], d_dout_b [E].  Every
 *                      output pointer may be NULL to skip it; with all four weight outputs NULL the workspace is not read.
 * Supported (rbx_fieldattn_supported): 2 <= F <= 48; E a multiple of 4 in [4, 32]; 1 <= h <= 8 dividing E with dh a multiple
 * of 4; dtype (the RBX_* code of every float tensor) RBX_F32; x, res and dy 16-byte aligned with strides that are multiples of
 * 4.  Anything else: RBX_ERR_UNSUPPORTED before any launch.  batch = 0 launches nothing.  No atomics, sums in a fixed order;
 * no call allocates or reads back: capturable.  Workgroups take up to 160 KiB of dynamic LDS. */
int rbx_fieldattn_supported(int32_t n_fields, int32_t dim, int32_t heads);
int rbx_fieldattn_fwd(const float* d_x, int64_t x_stride_b, int64_t x_stride_f, const float* d_in_w, const float* d_in_b,
                      const float* d_out_w, const float* d_out_b, const float* d_res, int64_t res_stride_b, int64_t res_stride_f,
                      int32_t relu, int64_t batch, int32_t n_fields, int32_t dim, int32_t heads, int32_t dtype, float p_drop,
                      uint64_t seed, const uint64_t* d_seed_add, float* d_y, float* d_attn, void* stream);
size_t rbx_fieldattn_bwd_workspace_size(int64_t batch, int32_t n_fields, int32_t dim, int32_t heads);
int rbx_fieldattn_bwd(const float* d_dy, int64_t dy_stride_b, int64_t dy_stride_f, const float* d_x, int64_t x_stride_b,
                      int64_t x_stride_f, const float* d_in_w, const float* d_in_b, const float* d_out_w, const float* d_y,
                      int32_t relu, int64_t batch, int32_t n_fields, int32_t dim, int32_t heads, int32_t dtype, float p_drop,
                      uint64_t seed, const uint64_t* d_seed_add, float* d_dx, float* d_dres, float* d_din_w, float* d_din_b,
                      float* d_dout_w, float* d_dout_b, void* d_workspace, size_t workspace_bytes, void* stream);

/* ---- FiGNN: one message-passing step of the field graph (csrc/rbx_fignn.hip; additions only, the version stays) --------------
 * Replaces, per layer of third_party/recbole/model/context_aware_recommender/fignn.py:119-137, the gathered [B, F^2, 2 A] concat
 * in front of Linear(2 A, 1), GraphLayer's two broadcast matmuls and bmm, nn.GRUCell on [B F, A] and the residual add.
 * B = batch, F = n_fields, A = dim.  Per sample, h, h0 [F, A] (h0: the residual and the graph's source), gates r, z, n:
 *   s_i = w_attn[:A] . h0_i     d_j = w_attn[A:] . h0_j     g[i, :] = softmax_j leaky_relu(s_i + d_j, 0.01), g[i, i] = 0
 *   hout_j = W_out[j] h_j       aggr_i = sum_j g[i, j] hout_j        a_i = W_in[i] aggr_i + bias_p
 *   r = sig(W_ir a + b_ir + W_hr h + b_hr)   z = sig(W_iz a + b_iz + W_hz h + b_hz)   n = tanh(W_in a + b_in + r (W_hn h + b_hn))
 *   h'_i = (1 - z) n + z h_i + h0_i
 * d_h, d_h0, d_dy [B, F, A], d_w_attn [2 A], d_w_out, d_w_in [F, A, A], d_bias_p [A], d_w_ih, d_w_hh [3 A, A], d_b_ih, d_b_hh
 * [3 A]: contiguous; h, h0 and w_attn 16-byte aligned (they are read four floats at a time).
 *   rbx_fignn_step_fwd  one launch.  A workgroup keeps hout and aggr of a tile of 16 (or 8) samples in LDS; the four matrix products
 *                       and g hout run on v_mfma_f32_16x16x4_f32, a field's matrices are fetched once per workgroup and tile.
 *                       Writes d_y [B, F, A] and, when not NULL, d_graph [B, F, F].
 *   rbx_fignn_step_bwd  one launch that recomputes the forward from its inputs and writes d_dh and d_dh0 [B, F, A] (separate
 *                       tensors: dh0 comes through the epilogue and through g), plus a tail launch that adds the per-workgroup
 *                       (dW_out, dW_in) and per-wavefront (the rest) partial rows of the workspace in a fixed order into
 *                       d_dw_attn [2 A], d_dw_out, d_dw_in [F, A, A], d_dbias_p [A], d_dw_ih, d_dw_hh [3 A, A], d_db_ih, d_db_hh
 *                       [3 A].  Every output pointer may be NULL to skip it; with all eight weight outputs NULL there are no
 *                       partial rows, no tail and no workspace.  rbx_fignn_step_bwd_workspace_size: at most 256 rows of
 *                       2 F A^2 and 1024 of 6 A^2 + 9 A floats whatever the batch (26 MiB at 39 x 16, 91 MiB at 39 x 32, 109 MiB at 48 x 32).
 * Supported (rbx_fignn_step_supported): 2 <= F <= 48 and A a multiple of 4 in [4, 32], every combination: where the backward's
 * two [F][16][A + 4] buffers do not fit in 160 KiB of LDS (from 46 fields at A = 20, 39 at 24, 34 at 28, 30 at 32) a tile is 8
 * samples.  dtype (the RBX_* code of every tensor) RBX_F32.  Anything else: RBX_ERR_UNSUPPORTED before any launch.  batch = 0
 * launches nothing.  No atomics, sums in a fixed order: equal bits run to run; no call allocates or reads back: capturable. */
int rbx_fignn_step_supported(int32_t n_fields, int32_t dim);
int rbx_fignn_step_fwd(const float* d_h, const float* d_h0, const float* d_w_attn, const float* d_w_out, const float* d_w_in,
                       const float* d_bias_p, const float* d_w_ih, const float* d_w_hh, const float* d_b_ih, const float* d_b_hh,
                       int64_t batch, int32_t n_fields, int32_t dim, int32_t dtype, float* d_y, float* d_graph, void* stream);
size_t rbx_fignn_step_bwd_workspace_size(int64_t batch, int32_t n_fields, int32_t dim);
int rbx_fignn_step_bwd(const float* d_dy, const float* d_h, const float* d_h0, const float* d_w_attn, const float* d_w_out,
                       const float* d_w_in, const float* d_bias_p, const float* d_w_ih, const float* d_w_hh, const float* d_b_ih,
                       const float* d_b_hh, int64_t batch, int32_t n_fields, int32_t dim, int32_t dtype, float* d_dh,
                       float* d_dh0, float* d_dw_attn, float* d_dw_out, float* d_dw_in, float* d_dbias_p, float* d_dw_ih,
                       float* d_dw_hh, float* d_db_ih, float* d_db_hh, void* d_workspace, size_t workspace_bytes, void* stream);

/* ---- FiBiNet: SENET gate and bilinear pair interaction (csrc/rbx_bilinear.hip; additions only, the version stays) -----------
 * Replaces, under third_party/rechub/basic/layers.py (SENETLayer, BiLinearInteractionLayer) and models/ranking/fibinet.py:31-38,
 * P = F (F - 1) / 2 nn.Linear calls on [B, 1, D] slices run twice per step, a torch.cat of 2 P pieces and a flatten.  B = batch,
 * F = fields, D = dim, R = reduced.  d_x is read at x[b x_stride_b + f x_stride_f + d], d < D.
 *   z[b, f] = mean_d x[b, f, d]    h = relu(w1 z)    a = act(w2 h)        d_w1 [R, F], d_w2 [F, R] contiguous (nn.Linear.weight,
 *                                                                         no bias); act: 0 = relu, 1 = sigmoid
 *   rbx_senet_gate_fwd  one launch, x read once; writes d_a [B, F] and d_h [B, R] (for the backward).
 *   rbx_senet_gate_bwd  from d_da [B, F], d_a and d_h as the forward wrote them: d_dx [B, F, D] contiguous = dz_f / D, written
 *                       (accumulate = 0) or added into what d_dx holds (accumulate != 0: a dx that rbx_bilinear_pairs_bwd
 *                       wrote); d_dw1 [R, F], d_dw2 [F, R]: one row per workgroup in the workspace
 *                       (rbx_senet_gate_bwd_workspace_size), added in ascending order by a second launch.
 *   out[b, p, :] = (x[b, i] W_m(p)) * x[b, j] for the pairs p = (i, j), i < j, in itertools.combinations order (i outer);
 *   out[b, P + p, :] = (a[b, i] a[b, j]) * out[b, p, :] when d_a [B, F] is not NULL -- the bilinear of x * a[..., None].
 *   kind: 0 = field_all (m = 0, M = 1 matrix), 1 = field_each (m = i, M = F), 2 = field_interaction (m = p, M = P); d_w
 *   [M, D, D] contiguous, a matrix stored [in, out] (transposed = 0) or [out, in] (transposed != 0: nn.Linear.weight).
 *   rbx_bilinear_pairs_fwd  one launch.  16 samples of x are staged in LDS once per workgroup, x_i W runs on
 *                           v_mfma_f32_16x16x4_f32 (exact fp32), W is read through L2.  Row r of sample b is written at
 *                           d_out[b out_stride_b + r D + d]: P rows, or 2 P with d_a.
 *   rbx_bilinear_pairs_bwd  d_dout addressed like d_out (dout_stride_b).  With g = dout1 + a_i a_j dout2 and L = x_i W
 *                           recomputed: dx_j += g L, dx_i += (g x_j) W^T, da_i += s a_j, da_j += s a_i with
 *                           s = sum_d dout2 L x_j, dW_m += x_i^T (g x_j).  Writes d_dx [B, F, D] and d_dw [M, D, D] (laid out as
 *                           d_w) in full and, with d_a and a non-NULL d_da, d_da [B, F].  Three launches: dx / da per tile of
 *                           16 samples; dW per (sample chunk, pair group) into the workspace
 *                           (rbx_bilinear_pairs_bwd_workspace_size: [chunks, P, D, D]); a tail that folds chunks and pairs onto
 *                           their matrix in ascending order.  Nothing of size [B, P, D] is allocated or expected.
 * Supported (rbx_senet_gate_supported / rbx_bilinear_pairs_supported; dtype = the RBX_* code of every float tensor): RBX_F32,
 * 2 <= F <= 64, D in {4, 8, 16, 32}, 1 <= R <= 32; x and dx 16-byte aligned, x strides multiples of 4.  Anything else:
 * RBX_ERR_UNSUPPORTED before any launch.  batch = 0 launches nothing.  No atomics, every sum in a fixed order: two runs give the
 * same bits.  Every launch goes to `stream`; no call allocates, clears, copies or reads back: capturable. */
int rbx_senet_gate_supported(int32_t fields, int32_t dim, int32_t reduced, int32_t dtype);
int rbx_senet_gate_fwd(const float* d_x, int64_t x_stride_b, int64_t x_stride_f, const float* d_w1, const float* d_w2,
                       int64_t batch, int32_t fields, int32_t dim, int32_t reduced, int32_t act, int32_t dtype, float* d_a,
                       float* d_h, void* stream);
size_t rbx_senet_gate_bwd_workspace_size(int64_t batch, int32_t fields, int32_t reduced);
int rbx_senet_gate_bwd(const float* d_da, const float* d_x, int64_t x_stride_b, int64_t x_stride_f, const float* d_w1,
                       const float* d_w2, const float* d_a, const float* d_h, int64_t batch, int32_t fields, int32_t dim,
                       int32_t reduced, int32_t act, int32_t dtype, int32_t accumulate, float* d_dx, float* d_dw1, float* d_dw2,
                       void* d_workspace, size_t workspace_bytes, void* stream);
int rbx_bilinear_pairs_supported(int32_t fields, int32_t dim, int32_t dtype);
int rbx_bilinear_pairs_fwd(const float* d_x, int64_t x_stride_b, int64_t x_stride_f, const float* d_w, const float* d_a,
                           int64_t batch, int32_t fields, int32_t dim, int32_t kind, int32_t transposed, int32_t dtype,
                           float* d_out, int64_t out_stride_b, void* stream);
size_t rbx_bilinear_pairs_bwd_workspace_size(int64_t batch, int32_t fields, int32_t dim);
int rbx_bilinear_pairs_bwd(const float* d_dout, int64_t dout_stride_b, const float* d_x, int64_t x_stride_b, int64_t x_stride_f,
                           const float* d_w, const float* d_a, int64_t batch, int32_t fields, int32_t dim, int32_t kind,
                           int32_t transposed, int32_t dtype, float* d_dx, float* d_da, float* d_dw, void* d_workspace,
                           size_t workspace_bytes, void* stream);

/* ---- DCN-V2: mixture of low-rank cross experts, one layer per call (csrc/rbx_crossmix.hip; additions only, the version stays) --
 * Replaces, under third_party/rechub/basic/layers.py (CrossNetMix) and models/ranking/dcn_v2.py, four matmuls and a Hadamard
 * product per expert, a torch.stack into [B, n, E] and a matmul with the softmax.  B = batch, E = experts, r = rank.  d_x0 and
 * d_xl are read at x[b stride + k], k < n; d_u, d_v [E, n, r], d_c [E, r, r], d_g [E, n] (the gates' Linear(n, 1) weights, one row
 * per expert), d_b [n], all contiguous.
 *   z_e = x_l . G_e    p = softmax_e(z)    h1_e = tanh(x_l V_e)    h2_e = tanh(h1_e C_e^T)
 *   mix = sum_e p_e (h2_e U_e^T) + b       out = x_l + x0 * mix
 *   rbx_crossmix_fwd  one launch: 16 rows of x_l staged in LDS once, [V | G^T] and U on v_mfma_f32_16x16x4_f32 (exact fp32), the
 *                     tanh / C / softmax stages in LDS; row b is written at d_out[b out_stride + k].  Nothing of size [B, E r] is
 *                     written.
 *   rbx_crossmix_bwd  d_dout addressed with dout_stride.  Recomputes h1, h2, p, mix from x_l.  Writes d_dxl (dxl_stride) = dout +
 *                     sum_e da1_e V_e^T + dz G, d_dx0 (dx0_stride) = dout * mix, d_du, d_dv, d_dc, d_db in full and d_dg; with
 *                     accumulate != 0, d_dx0 and d_dg are added to instead (the layers of a stack share x0 and G).  One row
 *                     launch, then per weight gradient a chunked batch reduction on the MFMA and a tail that adds the chunks in
 *                     ascending order; their [B, E r] operands live in the workspace (rbx_crossmix_bwd_workspace_size).
 * Supported (rbx_crossmix_supported; dtype = the RBX_* code of every tensor): RBX_F32, 1 <= n <= 640, 1 <= E <= 8, r in {4, 8, 16,
 * 32, 64}, E r <= 256.  Anything else: RBX_ERR_UNSUPPORTED before any launch.  batch = 0 launches nothing.  No atomics, every sum
 * in a fixed order: two runs give the same bits.  Every launch goes to `stream`; no call allocates, clears, copies or reads back:
 * capturable. */
int rbx_crossmix_supported(int32_t n, int32_t experts, int32_t rank, int32_t dtype);
int rbx_crossmix_fwd(const float* d_x0, int64_t x0_stride, const float* d_xl, int64_t xl_stride, const float* d_u,
                     const float* d_v, const float* d_c, const float* d_g, const float* d_b, int64_t batch, int32_t n,
                     int32_t experts, int32_t rank, int32_t dtype, float* d_out, int64_t out_stride, void* stream);
size_t rbx_crossmix_bwd_workspace_size(int64_t batch, int32_t n, int32_t experts, int32_t rank);
int rbx_crossmix_bwd(const float* d_dout, int64_t dout_stride, const float* d_x0, int64_t x0_stride, const float* d_xl,
                     int64_t xl_stride, const float* d_u, const float* d_v, const float* d_c, const float* d_g, const float* d_b,
                     int64_t batch, int32_t n, int32_t experts, int32_t rank, int32_t dtype, int32_t accumulate, float* d_dxl,
                     int64_t dxl_stride, float* d_dx0, int64_t dx0_stride, float* d_du, float* d_dv, float* d_dc, float* d_dg,
                     float* d_db, void* d_workspace, size_t workspace_bytes, void* stream);

/* ---- In-batch negatives: the band of the [B, B] cosine matrix (csrc/rbx_inbatch.hip; additions only, the version stays) ------
 * Replaces, under third_party/rechub/models/matching/youtube_sbc.py, torch.cosine_similarity(user.unsqueeze(1), item, dim=2) (a
 * [B, B, D] broadcast), "- log(sample_weight)" on the [B, B] result and the [index0, index1] gather that keeps B (n_neg + 1) of
 * its entries.  d_u, d_v are read at x[b stride + c], c < dim (16-byte aligned base, stride a multiple of 4); d_w [batch] or
 * NULL (no correction).  With j = (i + k) mod batch, k = 0 .. n_neg:
 *   ru_i = 1 / max(|u_i|, eps)    rv_j = 1 / max(|v_j|, eps)    scores[i, k] = (<u_i, v_j> ru_i rv_j - log w_j) inv_temperature
 *   rbx_inbatch_band_fwd  one launch: a workgroup stages 16 user rows and the 16 + n_neg item rows of their band in LDS once
 *                         (wrapped through mod batch), a lane group of 16 per row.  Writes d_scores[i scores_stride + k] and
 *                         d_ru, d_rv [batch] for the backward.
 *   rbx_inbatch_band_bwd  d_g read at g[i g_stride + k].  One launch: the same tile writes du_i (over the row's own band), dv_j and
 *                         dw_j = -inv_temperature sum_k g[(j - k) mod batch, k] / w_j (over the mirrored band); the cosines are
 *                         recomputed, a norm under eps is a constant denominator.  Any of d_du, d_dv, d_dw may be NULL (not
 *                         wanted); d_dw needs d_w.
 * Supported (rbx_inbatch_band_supported; dtype = the RBX_* code of every tensor): RBX_F32, dim a multiple of 4 in [4, 512],
 * 1 <= n_neg <= rbx_inbatch_band_max_neg(dim) = the largest n_neg <= 64 whose backward image, (16 + n_neg) (2 dim + 2 n_neg + 4)
 * floats, fits 160 KB of LDS (64 up to dim 128, 50 at 256, 22 at 512), and n_neg < batch.  Anything else: RBX_ERR_UNSUPPORTED
 * before any launch.  batch = 0 launches nothing.  No atomics, every sum in a fixed order: two runs give the same bits.  Every
 * launch goes to `stream`; no call allocates, clears, copies or reads back: capturable. */
int rbx_inbatch_band_max_neg(int32_t dim);
int rbx_inbatch_band_supported(int32_t dim, int32_t n_neg, int32_t dtype);
int rbx_inbatch_band_fwd(const float* d_u, int64_t u_stride, const float* d_v, int64_t v_stride, const float* d_w, int64_t batch,
                         int32_t dim, int32_t n_neg, float eps, float inv_temperature, int32_t dtype, float* d_scores,
                         int64_t scores_stride, float* d_ru, float* d_rv, void* stream);
int rbx_inbatch_band_bwd(const float* d_g, int64_t g_stride, const float* d_u, int64_t u_stride, const float* d_v,
                         int64_t v_stride, const float* d_w, const float* d_ru, const float* d_rv, int64_t batch, int32_t dim,
                         int32_t n_neg, float eps, float inv_temperature, int32_t dtype, float* d_du, int64_t du_stride,
                         float* d_dv, int64_t dv_stride, float* d_dw, void* stream);

/* ---- Caser: horizontal and vertical convolutions over a session block (csrc/rbx_caser.hip; additions only, the version stays) --
 * Replaces, under third_party/recbole/model/sequential_recommender/caser.py:121-137, a Conv2d, a ReLU and a max_pool1d per height
 * h = 1 .. L, the torch.cat of the L pieces, the vertical Conv2d and the second cat.  B = batch, d_x is read at
 * x[b x_stride_b + l x_stride_l + d], d < D (16-byte aligned base, strides multiples of 4).  w_h and b_h are HOST arrays of L device
 * pointers: w_h[h - 1] [n_h, h, D] and b_h[h - 1] [n_h], contiguous; they may be NULL when n_h = 0.  d_w_v [n_v, L], d_b_v [n_v]
 * contiguous, NULL when n_v = 0.  d_out [B, n_v D + n_h L] contiguous:
 *   out[b, v D + d]                 = b_v[v] + sum_l w_v[v, l] x[b, l, d]
 *   out[b, n_v D + (h - 1) n_h + f] = max_{t <= L - h} relu(b_h[h - 1][f] + sum_{i < h, d} w_h[h - 1][f, i, d] x[b, t + i, d])
 *   rbx_caser_fwd  one launch.  A workgroup stages the [L, D] blocks of 16 samples in LDS once (8 where 16 do not fit in 160 KiB,
 *                  L D + pad4(L) > 2552); every (h, t) window is a [16, h D] x [h D, n_h] product on v_mfma_f32_16x16x4_f32 (exact fp32)
 *                  with the filters read through L2, eight windows per pass; the running maximum and its t stay in registers; the
 *                  vertical rows come from the same LDS image.  Writes d_out and, when not NULL, d_win [B, L n_h] (int8): the
 *                  first maximal t of (h, f), or -1 where the ReLU is shut.
 *   rbx_caser_bwd  d_dout [B, n_v D + n_h L] contiguous, d_win as the forward wrote it.  Only the winning window of a (b, h, f)
 *                  carries gradient.  d_dx [B, L, D] contiguous (NULL: skipped): one launch, a thread per element with every sum
 *                  in ascending (h, f), then v.  The weight gradients -- d_dw_v [n_v, L], d_db_v [n_v] and the host arrays dw_h,
 *                  db_h of L device pointers laid out as w_h, b_h (all four NULL: skipped) -- take two launches: a thread per
 *                  gradient element and run of samples into the workspace (rbx_caser_bwd_workspace_size: [runs <= 32][n_h D L
 *                  (L + 1) / 2 + n_h L + n_v L + n_v] floats), and a tail that adds the runs in ascending order.
 * Supported (rbx_caser_supported): 1 <= L <= 50, D a multiple of 4 in [4, 64], 0 <= n_h <= 16, 0 <= n_v <= 16, n_h + n_v > 0.
 * dtype (the RBX_* code of every float tensor) RBX_F32.  Anything else: RBX_ERR_UNSUPPORTED before any launch.  batch = 0 launches
 * nothing.  No atomics, every sum in a fixed order: two runs give the same bits.  Every launch goes to `stream`; no call
 * allocates, clears, copies or reads back: capturable. */
int rbx_caser_supported(int32_t L, int32_t D, int32_t n_h, int32_t n_v);
int rbx_caser_fwd(const float* d_x, int64_t x_stride_b, int64_t x_stride_l, const float* d_w_v, const float* d_b_v,
                  const void* const* w_h, const void* const* b_h, int64_t batch, int32_t L, int32_t D, int32_t n_h, int32_t n_v,
                  int32_t dtype, float* d_out, int8_t* d_win, void* stream);
size_t rbx_caser_bwd_workspace_size(int64_t batch, int32_t L, int32_t D, int32_t n_h, int32_t n_v);
int rbx_caser_bwd(const float* d_dout, const float* d_x, int64_t x_stride_b, int64_t x_stride_l, const float* d_w_v,
                  const void* const* w_h, const int8_t* d_win, int64_t batch, int32_t L, int32_t D, int32_t n_h, int32_t n_v,
                  int32_t dtype, float* d_dx, float* d_dw_v, float* d_db_v, void* const* dw_h, void* const* db_h,
                  void* d_workspace, size_t workspace_bytes, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* RECBOX_HIP_H */
