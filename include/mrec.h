/*
 * mrec.h -- C ABI of libmrec.so, the MI355X (gfx950) embedding-lookup +
 * feature-interaction hot path.
 *
 * The reference (Troublem1/PyTorchRec) is pure Python; its hot path is the ATen
 * op sites listed in SURVEY.md §2b, reached from IModel.train_step
 * (torchrec/model/IModel.py:116-125).  Each entry point below names the
 * reference interface it replaces.  The Python side (pytorchrec_amd/_mrec.py)
 * binds these with ctypes; INTEGRATION.md shows the binding.
 *
 * Conventions (all entry points):
 *   - Every buffer is a caller-owned device pointer (torch caching allocator).
 *     The library keeps no pointer past return and allocates nothing; scratch
 *     is passed in as a workspace sized by a *_workspace_size query.
 *   - Arrays documented as HOST are read during the call only.
 *   - Work is enqueued on `stream` (a hipStream_t); no call synchronises the
 *     device, so every call is safe inside hipStreamBeginCapture (hipGraphs).
 *   - Return value is an mrec_status; on error mrec_last_error() (thread-local)
 *     describes it.  No C++ exception crosses the ABI.
 *   - Out-of-range ids never fault: the kernel substitutes a zero row (forward)
 *     or skips the lookup (backward) and sets *d_oob_flag (device int32, may be
 *     NULL) to 1.  The Python wrapper turns the flag into IndexError in its
 *     checked mode, matching nn.Embedding.
 */
#ifndef MREC_H
#define MREC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MREC_ABI_VERSION 40
#define MREC_MAX_TABLES 64      /* tables per table bank / per call */
#define MREC_BWD_MAX_BATCH 8192  /* lookups per table per plan/apply call */
#define MREC_BWD_HASH_MAX_BATCH 4096  /* batches up to this use the hash plan */
#define MREC_NEG_MAX_ATTEMPTS 32  /* draws per output of mrec_neg_sample before it gives up */

typedef enum {
  MREC_OK = 0,
  MREC_EINVAL = 1, /* bad argument (null pointer, size, dtype combination) */
  MREC_EOOB = 2,   /* reserved: host-detected out-of-range id */
  MREC_EHIP = 3,   /* HIP runtime error (launch failure, ...) */
  MREC_ERCCL = 4,  /* reserved for RCCL errors */
  MREC_ENOSPC = 5  /* workspace too small */
} mrec_status;

typedef enum { MREC_F32 = 0, MREC_BF16 = 1, MREC_I32 = 2, MREC_I64 = 3 } mrec_dtype;

typedef void *mrec_stream; /* hipStream_t */

/*
 * A table bank: F embedding tables packed row-wise into one device buffer
 * [total_rows, row_stride] of `dtype`.  Table f occupies rows
 * [row_offset[f], row_offset[f] + rows[f]).  Row r holds the embedding
 * v[0..dim) and, when has_w, the first-order weight w at column `dim`
 * (SURVEY.md §7 hard part 1: "[v(16) | w | pad]").  row_stride*sizeof(dtype)
 * must be a power of two in [16, 256] bytes (64 B for bf16 D=16 + w).
 * Replaces F x torch.nn.Embedding(rows_f, dim) (+ Embedding(rows_f, 1) biases)
 * built in IModel._init_weights (FunkSVD.py:39-41, SVDPP.py:36-42).
 */
struct mrec_optim_s; /* mrec_optim: the fused row-sparse optimizer state, below */

typedef struct {
  void *data;                 /* device */
  const int64_t *row_offset;  /* HOST [n_tables] */
  const int64_t *rows;        /* HOST [n_tables] */
  int32_t n_tables;
  int32_t dim;
  int32_t row_stride; /* elements */
  int32_t has_w;
  mrec_dtype dtype; /* MREC_F32 or MREC_BF16 */
  /* HOST, may be NULL: optimizer state of the fused updates MREC_BWD_ADAGRAD /
   * _ROWWISE_ADAGRAD / _ADAM (the state belongs to the table like its rows) */
  const struct mrec_optim_s *optim;
} mrec_table_bank;

/*
 * Per-field categorical ids: field f of sample b is at
 * field_ptr[f][b * stride] (int32 or int64).  field_ptr is a HOST array of
 * n_tables device pointers, so the batch dict's per-feature tensors
 * (CategoricalColumnWithIdentity.get_feature_data, .py:20-22) are read in place
 * and a stacked [B, F] tensor is field_ptr[f] = base + f, stride = F.
 */
typedef struct {
  const void *const *field_ptr; /* HOST [n_tables] of device pointers */
  mrec_dtype dtype;             /* MREC_I32 or MREC_I64 */
  int64_t stride;               /* elements between samples */
  /* chunked addressing (0 = off): element b of a field sits at
   * field_ptr[f][(b / chunk) * chunk_stride + b % chunk] — the owner-side view of
   * an all-to-all receive buffer [source][table][slot] (see mrec_shard_*) */
  int64_t chunk;
  int64_t chunk_stride;
  int32_t pad_negative; /* negative ids are padding slots: skipped, never flagged OOB */
} mrec_ids;

int mrec_abi_version(void);
const char *mrec_last_error(void);

/* ------------------------------------------------------------------------- */
/* Forward                                                                   */
/* ------------------------------------------------------------------------- */

/*
 * Multi-table gather: out[b, f*dim + d] = bank[row_offset[f] + id[f][b], d]
 * (bit-exact copy when out_dtype == bank dtype; bf16->f32 widening is exact).
 * Row stride of `out` is out_ld elements.  If w_out != NULL (bank must have_w)
 * w_out[b*n_tables + f] = w (fp32).
 * Replaces nn.Embedding forward = aten::embedding -> index_select
 * (FunkSVD.py:47-48, NCF.py:62-65).
 */
mrec_status mrec_emb_gather_fwd(const mrec_table_bank *bank, const mrec_ids *ids, int64_t batch,
                                void *out, mrec_dtype out_dtype, int64_t out_ld, float *w_out,
                                int32_t *d_oob_flag, mrec_stream stream);

/* pooled (multi-valued) lookups, ABI 30 */
#define MREC_POOL_SUM 0   /* s = 1 */
#define MREC_POOL_MEAN 1  /* s = 1 / n, n = the bag's valid count */
#define MREC_POOL_SQRTN 2 /* s = 1 / sqrt(n): the reference's SVD++ history term (SVDPP.py:49-55) */
#define MREC_POOL_PAD_ZERO 0     /* id 0 is padding (the reference's `iids > 0` mask, SVDPP.py:50);
                                    a negative id is out of range, as nn.Embedding raises on it
                                    before the mask applies */
#define MREC_POOL_PAD_NEGATIVE 1 /* a negative id is padding, id 0 is a real row: the
                                    pad_negative convention of mrec_ids */

/*
 * Pooled lookup (ABI 30): a field of a sample is a BAG of bag_len ids -- field f, bag
 * b, position j at field_ptr[f][b * ids->stride + j], stride >= bag_len, every field
 * of the call with the same bag_len -- and
 *   out[b, f*dim + d]      = s_bf * sum_{valid j} bank[row_offset[f] + id_bfj, d]
 *   bag_scale[b*F + f]     = s_bf   (fp32, required: the backward's per-bag factor)
 *   w_out[b*F + f]         = s_bf * sum_{valid j} w   (when non-NULL; bank must have_w)
 *   lookup_ids[f][b*bag_len + j] = id of a valid lookup, -1 for padding and for an
 *                            out-of-range id (nullable; int32 [F][n_bags * bag_len]:
 *                            the padded id view, pad_negative = 1, that the backward
 *                            plan consumes -- built in the gather launch as
 *                            mrec_din_gather builds its ids)
 * The sum is fp32 in ascending position order from a -0.0f accumulator (bitwise
 * reproducible), then one multiply by s and one rounding into out_dtype (F32 / BF16).
 * An empty bag gives a zero row and s = 0 (the reference: 0 / sqrt(0) = NaN).  An
 * out-of-range id sets *d_oob_flag, contributes nothing and is never dereferenced.
 * A bank under the lazy fused Adam is read as of the last step, like every gather.
 * Replaces implicit_i_embeddings(iids) + mask + sum + / sqrt(count), SVDPP.py:49-55.
 */
mrec_status mrec_emb_pool_fwd(const mrec_table_bank *bank, const mrec_ids *ids, int64_t n_bags,
                              int32_t bag_len, int32_t pool_mode, int32_t pad_mode, void *out,
                              mrec_dtype out_dtype, int64_t out_ld, float *w_out,
                              float *bag_scale, int32_t *lookup_ids, int32_t *d_oob_flag,
                              mrec_stream stream);

/* flags for mrec_interact_fwd */
#define MREC_INTERACT_FM2 1         /* add 1/2 sum_d[(sum_f v)^2 - sum_f v^2] */
#define MREC_INTERACT_FIRST_ORDER 2 /* add sum_f w[id_f] (bank must have_w) */

/*
 * Fused gather + interaction + deep-input builder, one wave per sample, the
 * per-sample [F, D] block held in registers and reduced with wave shuffles:
 *   x0[b, :]   = [ v_0 .. v_{F-1} (F*dim) | dense[b, 0..n_dense) | 0 .. ]   (x0_cols wide)
 *   logit[b]   = bias + dense[b].dense_w + (FM2 ? fm2(v) : 0) + (FIRST_ORDER ? sum_f w : 0)
 *   fm_sum[b,:] = sum_f v_f   (fp32, saved for the backward; may be NULL)
 * x0 may be NULL (pure FM, config C1); dense may be NULL when n_dense==0, dense_w
 * NULL drops the dense first-order term (DCN-v2 feeds dense only to x0);
 * bias is a device float[1] (may be NULL = 0).  x0_dtype F32 or BF16.
 * Replaces: nn.Embedding gathers + torch.cat + the FM mul/sum + bias
 * embeddings (FunkSVD.py:47-51, SVDPP.py:57-66, NCF.py:62-70).
 */
mrec_status mrec_interact_fwd(const mrec_table_bank *bank, const mrec_ids *ids, int64_t batch,
                              const float *dense, int32_t n_dense, int64_t dense_ld,
                              const float *dense_w, const float *bias, int32_t flags, void *x0,
                              mrec_dtype x0_dtype, int64_t x0_ld, int32_t x0_cols, float *logit,
                              float *fm_sum, int32_t *d_oob_flag, mrec_stream stream);

/*
 * Standalone FM second order on a dense [B, F, D] fp32 tensor (row-major),
 * y[b] = 1/2 sum_d[(sum_f v)^2 - sum_f v^2]; bwd dv = dy[b] (S_d - v_fd).
 * FunkSVD.py:51 is the F = 2 case.
 */
mrec_status mrec_fm2_fwd(const float *v, int64_t batch, int32_t fields, int32_t dim, float *y,
                         mrec_stream stream);
mrec_status mrec_fm2_bwd(const float *v, const float *dy, int64_t batch, int32_t fields,
                         int32_t dim, float *dv, mrec_stream stream);

/* ------------------------------------------------------------------------- */
/* Backward: embedding scatter-add                                           */
/* ------------------------------------------------------------------------- */

typedef enum {
  MREC_BWD_DENSE_GRAD = 0, /* grad[row] += sum g  (grad laid out like the bank, dtype of bank;
                              caller zero-fills; == aten::embedding_dense_backward) */
  MREC_BWD_SGD = 1,        /* bank[row] -= lr * sum g, round-to-nearest-even */
  MREC_BWD_SGD_SR = 2,     /* bank[row] -= lr * sum g, stochastic rounding (bf16 banks) */
  /* fused optimizers (bank->optim required; fp32 math on the row, one rounding of
   * the result into a bf16 bank).  g = the row's summed gradient this step. */
  MREC_BWD_ADAGRAD = 3,    /* torch.optim.Adagrad (lr_decay 0, initial accumulator 0, no
                              weight decay): s += g^2, w -= lr g / (sqrt(s) + eps);
                              rows not looked up are unchanged, exactly as in the dense
                              optimizer */
  MREC_BWD_ROWWISE_ADAGRAD = 4, /* one accumulator per row for the vector (s += mean_d g_d^2)
                              and one for the first-order weight: w_d -= lr g_d /
                              (sqrt(s) + eps) */
  MREC_BWD_ADAM = 5        /* dense-compatible Adam / AdamW (reference optim/AdamW.py:21-61,
                              torch.optim.Adam): a row brought from step row_step[row] to t
                              runs the zero-gradient steps it missed (momentum decay, L2
                              decay, decoupled decay) in order, then step t with g; rows
                              not looked up catch up at their next lookup or at
                              mrec_emb_optim_flush, after which the table and state equal
                              dense Adam's */
} mrec_bwd_mode;

#define MREC_OPT_DECOUPLED_WD 1       /* AdamW: w -= lr * wd * w after the step (reference
                                         AdamW.py:58-59), eps added to sqrt(v) before the
                                         bias correction of the step size (AdamW.py:50-56);
                                         else torch.optim.Adam: L2 decay g += wd * w, eps
                                         after sqrt(v / (1 - beta2^t)) */
#define MREC_OPT_NO_BIAS_CORRECTION 2 /* AdamW(correct_bias=False) */

typedef struct mrec_optim_s {
  int32_t kind;        /* the optimizer's mrec_bwd_mode (ADAGRAD / ROWWISE_ADAGRAD / ADAM) */
  float lr;            /* ADAM: lr of the zero-gradient catch-up steps run when a stale row is
                          READ (forward gathers); the apply's own lr argument steps the rows it
                          updates.  Exact while lr is constant: flush before changing it */
  double beta1, beta2; /* double: the bias corrections 1 - beta^t are formed in double, as the
                          dense optimizers do on the host */
  float eps, weight_decay;
  float grad_scale;   /* the optimizer sees grad_scale * g (a row-sharded owner: 1 / world) */
  int32_t flags;      /* MREC_OPT_* */
  float *state0;      /* ADAGRAD: sum of g^2 [total_rows, state_ld]; ROWWISE_ADAGRAD: [total_rows, 2]
                         (vector, first-order weight); ADAM: exp_avg [total_rows, state_ld] */
  float *state1;      /* ADAM: exp_avg_sq [total_rows, state_ld] */
  int32_t *row_step;  /* ADAM: the step each row is current to [total_rows] (zero at start) */
  const int64_t *d_t; /* ADAM: device step counter t, advanced by the caller before each step's
                         apply (stream-ordered, so it stays correct under graph replay) */
  int64_t state_ld;   /* floats per state row: mrec_emb_optim_state_ld */
} mrec_optim;

/* floats per optimizer-state row for a bank of `dim` (+ first-order weight) */
int64_t mrec_emb_optim_state_ld(int32_t dim, int32_t has_w);

/*
 * MREC_BWD_ADAM: bring every row not updated at the current step t (*d_t) up to t
 * by zero-gradient steps, so the table and state equal dense Adam's (call before
 * evaluation, checkpointing or a change of lr).  Other modes: no-op.
 */
mrec_status mrec_emb_optim_flush(const mrec_table_bank *bank, mrec_bwd_mode mode, float lr,
                                 mrec_stream stream);

/*
 * Bytes of workspace mrec_emb_bwd needs for `batch` lookups per table.
 */
size_t mrec_emb_bwd_workspace_size(int32_t n_tables, int64_t batch);

/*
 * Plan of the embedding backward: per table the lookups are grouped by row (an
 * LDS hash table for batch <= MREC_BWD_HASH_MAX_BATCH, a stable LDS radix sort
 * up to MREC_BWD_MAX_BATCH).  Depends only on the ids, so it can run as soon as
 * the batch is resident (or inside another launch: mrec_interact_fwd_ex,
 * mrec_shard_gather_wire).  If d_step (device uint64, may be NULL) is given the plan
 * increments it once, so a graph replayed step after step still draws fresh
 * stochastic-rounding bits.
 *
 * Workspace layout rule (ABI 28).  The plan writes the HASH layout when batch <=
 * MREC_BWD_HASH_MAX_BATCH, or when the ids are a padded exchange view
 * (mrec_ids.pad_negative) of batch <= MREC_BWD_MAX_BATCH entries; else the SORTED
 * layout.  An apply reads the hash layout when batch <= MREC_BWD_HASH_MAX_BATCH or
 * when its gradients are given (mrec_emb_bwd_apply_given with g_occ, _wire), else
 * the sorted one.  So a padded plan of more than MREC_BWD_HASH_MAX_BATCH entries is
 * consumed only by the given-gradient applies.  Every plan entry (this one, the
 * mrec_plan_job of mrec_interact_fwd_ex / mrec_shard_gather_wire(_ex)) records
 * {layout, batch, n_tables} for its workspace address when it is issued (host side;
 * the same tag, (batch << 2) | layout, is stamped into the device headers), and every
 * apply (mrec_emb_bwd_apply, _ex, _given, _rec, _wire) returns MREC_EINVAL, with
 * mrec_last_error naming both layouts, when the workspace's last plan wrote another
 * layout, batch or table count, or when no plan was issued into it.  Batch 0 reads
 * nothing and is not checked.  (The reference's autograd backward cannot be
 * mis-paired: IModel.py:123; misuse raises: IModel.py:101-108.)
 */
mrec_status mrec_emb_bwd_plan(const mrec_table_bank *bank, const mrec_ids *ids, int64_t batch,
                              void *workspace, size_t ws_bytes, int32_t *d_oob_flag,
                              uint64_t *d_step, mrec_stream stream);

/* an embedding-backward hash plan (arguments of mrec_emb_bwd_plan) */
typedef struct {
  const mrec_table_bank *bank;
  const mrec_ids *ids;
  int64_t batch; /* 1 .. MREC_BWD_HASH_MAX_BATCH */
  void *workspace;
  size_t ws_bytes;
  int32_t *d_oob_flag;
  uint64_t *d_step;
} mrec_plan_job;

/*
 * mrec_interact_fwd plus the embedding-backward hash plan of `plan` (may be NULL;
 * batch <= MREC_BWD_HASH_MAX_BATCH) in leading workgroups of the same launch: the
 * plan depends only on the ids, and beside the latency-bound interaction it costs
 * no kernel boundary.  Same outputs as the two calls made separately.
 */
mrec_status mrec_interact_fwd_ex(const mrec_table_bank *bank, const mrec_ids *ids, int64_t batch,
                                 const float *dense, int32_t n_dense, int64_t dense_ld,
                                 const float *dense_w, const float *bias, int32_t flags, void *x0,
                                 mrec_dtype x0_dtype, int64_t x0_ld, int32_t x0_cols, float *logit,
                                 float *fm_sum, int32_t *d_oob_flag, const mrec_plan_job *plan,
                                 mrec_stream stream);

/*
 * The compact exchange's received rows as wire records (ABI 28): record
 * p * cap_rows + pref[p][f] + j answers slot (p * n_tables + f) * cap + j of the ids
 * message `hdr` (parts x (n_tables * cap + n_tables) int32, the per-table counts
 * last; pref[p][f] = the running sum of part p's counts of the tables before f).
 */
typedef struct {
  const void *wire;     /* [parts][cap_rows] records of rec_bytes (4-B multiple, bf16 row + w) */
  int32_t rec_bytes;
  const int32_t *hdr;   /* the ids message the sender sent (mrec_shard_bucketize_dedup) */
  int32_t parts, cap, cap_rows;
  int32_t *pref;        /* out, nullable: [parts][n_tables] prefixes (mrec_emb_bwd_apply_rec) */
  int32_t *d_overflow;  /* nullable: bit 1 set when a part's counts exceed cap_rows */
} mrec_wire_rows;

/*
 * mrec_interact_fwd_ex over the compact exchange's received records without the
 * unpack launch: `bank` is the sender's slot rows (every table = the whole
 * parts x n_tables x cap slot range, row offset 0; bf16, 64-B rows) and `ids` the
 * lookups' slots (mrec_shard_bucketize_dedup pos).  Each lookup's row is read from its
 * record and also written into its slot row -- the bytes mrec_shard_wire_unpack_ex
 * writes there (the record, zeros past it), which the sender's backward reads -- and
 * the launch writes the parts' prefixes to rows->pref.  Same outputs as
 * mrec_shard_wire_unpack_ex followed by mrec_interact_fwd_ex.  (ABI 28)
 */
mrec_status mrec_interact_fwd_rec(const mrec_table_bank *bank, const mrec_ids *ids, int64_t batch,
                                  const float *dense, int32_t n_dense, int64_t dense_ld,
                                  const float *dense_w, const float *bias, int32_t flags, void *x0,
                                  mrec_dtype x0_dtype, int64_t x0_ld, int32_t x0_cols, float *logit,
                                  float *fm_sum, int32_t *d_oob_flag, const mrec_plan_job *plan,
                                  const mrec_wire_rows *rows, mrec_stream stream);

/*
 * Gradient sources of lookup (b, f) (each may be NULL = 0):
 *   g_v[d] = dx[b, f*dim + d]                                (dx: F32/BF16, row stride dx_ld)
 *          + dfm[b] * (fm_sum[b, d] - v[b, f*dim + d])      (FM2 backward; v read from x0)
 *   g_w    = dw[b]                                          (first-order backward)
 * Segment sums are fp32 in ascending sample order (bitwise reproducible), then
 * applied per unique row as `mode` says.  Stochastic rounding draws its bits from
 * hash(seed + *d_step, row, column) (d_step may be NULL = 0).
 * Replaces aten::embedding_dense_backward + the dense optimizer step
 * (IModel.py:120-124).
 */
mrec_status mrec_emb_bwd_apply(const mrec_table_bank *bank, int64_t batch, const void *workspace,
                               size_t ws_bytes, const void *dx, mrec_dtype dx_dtype, int64_t dx_ld,
                               const float *dfm, const float *fm_sum, const void *x0,
                               mrec_dtype x0_dtype, int64_t x0_ld, const float *dw,
                               mrec_bwd_mode mode, float lr, uint64_t seed,
                               const uint64_t *d_step, void *grad, mrec_stream stream);

/*
 * Large-batch embedding backward (more than MREC_BWD_MAX_BATCH lookups per table,
 * e.g. DIN's B x L history lookups; banks of <= 2^24 rows in total): a device-wide
 * counting sort by row (plan) and ONE update per row with the sum of all its
 * lookups (apply) — what aten::embedding_dense_backward + the optimizer step do
 * for nn.Embedding (reached from FunkSVD.py:39-41 style
 * tables), instead of one SGD step per 8192-lookup chunk.  Rows hit <= 16 times
 * are summed in ascending sample order (as mrec_emb_bwd_apply); hotter rows are
 * summed in 64-bit fixed point scaled to the row's largest gradient (exact,
 * order-independent, bitwise reproducible).  Same arguments and modes as
 * mrec_emb_bwd_plan / mrec_emb_bwd_apply; `batch` = lookups per table.
 * The first mrec_emb_bwd_large_zero_bytes() bytes of the workspace must be zero
 * before its first use (torch.zeros); every apply leaves them zero again.
 */
size_t mrec_emb_bwd_large_workspace_size(const mrec_table_bank *bank, int64_t batch);
size_t mrec_emb_bwd_large_zero_bytes(const mrec_table_bank *bank, int64_t batch);
mrec_status mrec_emb_bwd_large_plan(const mrec_table_bank *bank, const mrec_ids *ids, int64_t batch,
                                    void *workspace, size_t ws_bytes, int32_t *d_oob_flag,
                                    mrec_stream stream);
mrec_status mrec_emb_bwd_large_apply(const mrec_table_bank *bank, int64_t batch,
                                     const void *workspace, size_t ws_bytes, const void *dx,
                                     mrec_dtype dx_dtype, int64_t dx_ld, const float *dfm,
                                     const float *fm_sum, const void *x0, mrec_dtype x0_dtype,
                                     int64_t x0_ld, const float *dw, mrec_bwd_mode mode, float lr,
                                     uint64_t seed, const uint64_t *d_step, void *grad,
                                     mrec_stream stream);
/*
 * mrec_emb_bwd_large_plan + mrec_emb_bwd_large_apply in one call (ABI 20).  For
 * batches of <= 2M lookups over banks whose rows hash into at most 512 per bucket
 * (NB = batch * n_tables / 256 buckets, a power of two <= 8192), the BUCKETED plan
 * runs: lookups are partitioned by a multiplicative hash of their row (bucket
 * histograms per 8192-lookup chunk, per-bucket prefix, scatter: no per-row global
 * atomics), then one workgroup per bucket groups its rows in LDS and updates them
 * in place — rows hit <= 16 times summed in ascending sample order by one worker,
 * 17..2048 times in 64-bit fixed point by a wave (the same arithmetic, hence the
 * same bits, as the two-call path), and longer segments through the chunked
 * fixed-point kernels.  Otherwise (or with MREC_LG_ATOMIC_PLAN set) it is the
 * two calls.  Same arguments as the two calls; same workspace.
 */
mrec_status mrec_emb_bwd_large_fused(const mrec_table_bank *bank, const mrec_ids *ids,
                                     int64_t batch, void *workspace, size_t ws_bytes,
                                     int32_t *d_oob_flag, const void *dx, mrec_dtype dx_dtype,
                                     int64_t dx_ld, const float *dfm, const float *fm_sum,
                                     const void *x0, mrec_dtype x0_dtype, int64_t x0_ld,
                                     const float *dw, mrec_bwd_mode mode, float lr, uint64_t seed,
                                     const uint64_t *d_step, void *grad, mrec_stream stream);

/*
 * Kernel clock (ABI 25, measurement only: bench.py's in-step roofline).  With a
 * buffer set, every launch of the step's hot kernels -- mrec_interact_fwd_ex (the
 * plan-fused launch), mrec_emb_bwd_apply(_ex) (hash layout), mrec_tower_fwd_bwd,
 * mrec_tower_dw -- takes the next slot (in launch order; a HIP graph captured
 * meanwhile keeps its slots) and runs a clocked instantiation of its kernel
 * (the production instantiations carry no clock code).  Every wave records its
 * start and its end (after its stores are acknowledged) into shard
 * (global wave index % MREC_KCLOCK_SHARDS) of its slot:
 * buf[slot][MREC_KCLOCK_SHARDS][MREC_KCLOCK_SHARD_U64] u64, element 0 = min start,
 * element 1 = max end, s_memrealtime (100 MHz ticks); one 128-B line per shard
 * keeps the waves' atomics apart.  The caller fills starts with ~0 and ends with
 * 0 before each run and reduces min / max over the shards.  NULL turns it off
 * (the default).  Not thread-safe; host-side counter only.
 */
#define MREC_KCLOCK_SHARDS 4096
#define MREC_KCLOCK_SHARD_U64 16
void mrec_kernel_clock(void *buf, int32_t n_slots);
int32_t mrec_kernel_clock_used(void);

/*
 * Per-lookup gradients GIVEN by the caller instead of computed from dx / dfm (the
 * owner side of the row-sharded exchange).  The lookups are an
 * exchange view (mrec_ids with chunk = the entries per part): entry b of table f
 * sits in part p = b / chunk at j = b % chunk.  Exactly one source:
 *   g_occ: fp32 rows [.., g_ld], entry (p, f, j) at row p * chunk_stride + f * chunk
 *          + j (the slot exchange's received gradient slots);
 *   wire:  records of rec_bytes (wire_dtype BF16 / F32), entry (p, f, j) at record
 *          p * cap_rows + pref[p * n_tables + f] + j (the compact exchange; an entry
 *          past its part's cap_rows records gets a zero gradient).
 */
typedef struct {
  const float *g_occ;
  int64_t g_ld;
  int64_t chunk;
  int64_t chunk_stride;
  const void *wire;
  int32_t rec_bytes;
  mrec_dtype wire_dtype;
  const int32_t *pref;
  int32_t cap_rows;
} mrec_given_grads;

/*
 * Byte offset, inside the large-batch workspace, of an int32 STICKY error word
 * (ABI 25).  The fused path's huge segments (a row hit > 2048 times) are summed in
 * one launch of three dependent phases whose work items are dequeued in phase
 * order (no co-residency assumed, so a phase wait always ends); its waits are still
 * bounded, and a wait that ran out (a hardware stall; or MREC_LG_HUGE_TEST_STALL,
 * a test-only knob that makes them unreachable) leaves the rows of that launch's
 * huge segments un-updated and sets this word to 1; a bank of more than 2^24 rows
 * (only the bucketed plan) whose bucket holds more distinct rows than its LDS hash
 * sets 2 (those rows un-updated).  No kernel clears it:
 * the caller reads it at a sync point of its choosing, raises, and zeroes it.
 */
size_t mrec_emb_bwd_large_error_offset(void);

struct mrec_gemm_call_s; /* mrec_gemm_call, defined with the GEMM entry points below */

/*
 * mrec_emb_bwd_large_fused plus up to 6 deferred split-K weight-gradient reductions
 * (phase MREC_GEMM_REDUCE, as for mrec_emb_bwd_apply_ex) run by workgroups after
 * the bucket kernel's own (ABI 24): DIN's top-tower dW reduce + fused SGD leaves
 * its standalone launch.  They must not touch what the update reads or writes.  On
 * the two-call path (and for batch 0) they run as one mrec_gemm_multi after it.
 */
mrec_status mrec_emb_bwd_large_fused_ex(const mrec_table_bank *bank, const mrec_ids *ids,
                                        int64_t batch, void *workspace, size_t ws_bytes,
                                        int32_t *d_oob_flag, const void *dx, mrec_dtype dx_dtype,
                                        int64_t dx_ld, const float *dfm, const float *fm_sum,
                                        const void *x0, mrec_dtype x0_dtype, int64_t x0_ld,
                                        const float *dw, mrec_bwd_mode mode, float lr,
                                        uint64_t seed, const uint64_t *d_step, void *grad,
                                        int32_t n_reduce, const struct mrec_gemm_call_s *reduce,
                                        mrec_stream stream);

/*
 * mrec_emb_bwd_large_fused_ex over GIVEN per-lookup gradients (ABI 25; the owner
 * side of the row-sharded exchange when an exchange view exceeds the hash plan's
 * MREC_BWD_MAX_BATCH entries per table: large W * cap, Zipf).  `ids` is the exchange
 * view of the received ids (pad_negative: padding slots skipped), `batch` its
 * entries per table.  Same sums and update arithmetic as every large-batch path.
 */
mrec_status mrec_emb_bwd_large_fused_given(const mrec_table_bank *bank, const mrec_ids *ids,
                                           int64_t batch, void *workspace, size_t ws_bytes,
                                           int32_t *d_oob_flag, const mrec_given_grads *given,
                                           mrec_bwd_mode mode, float lr, uint64_t seed,
                                           const uint64_t *d_step, void *grad, int32_t n_reduce,
                                           const struct mrec_gemm_call_s *reduce,
                                           mrec_stream stream);

/*
 * mrec_emb_bwd_apply plus up to 6 deferred split-K weight-gradient reductions
 * (mrec_gemm_call with phase MREC_GEMM_REDUCE, e.g. the first MLP layer's dW +
 * fused SGD) run by extra workgroups of the same launch.  They must not touch
 * what the apply reads or writes.  A HIP graph runs the step's kernels one after
 * another, so a reduction launched on its own costs a full kernel on the
 * critical path.
 */
mrec_status mrec_emb_bwd_apply_ex(const mrec_table_bank *bank, int64_t batch,
                                  const void *workspace, size_t ws_bytes, const void *dx,
                                  mrec_dtype dx_dtype, int64_t dx_ld, const float *dfm,
                                  const float *fm_sum, const void *x0, mrec_dtype x0_dtype,
                                  int64_t x0_ld, const float *dw, mrec_bwd_mode mode, float lr,
                                  uint64_t seed, const uint64_t *d_step, void *grad,
                                  int32_t n_reduce, const struct mrec_gemm_call_s *reduce,
                                  mrec_stream stream);

/*
 * The backward of mrec_emb_pool_fwd (ABI 30; the gradient of SVDPP.py:49-55): the
 * arguments of mrec_emb_bwd_apply_ex / mrec_emb_bwd_large_fused_ex over batch =
 * n_bags * bag_len lookups -- planned from the forward's lookup_ids view -- whose
 * gradients come through a bag index: lookup i of table f takes
 *   g_v = bag_scale[bb*F + f] * dx[bb*dx_ld + f*dim + d],  g_w = bag_scale[bb*F + f] * dw[bb]
 * with bb = i / bag_len (one fp32 multiply; dx / dw hold one row per bag, so the
 * bag's gradient row is never expanded to bag_len copies).  Everything else is the
 * plain entry's: layouts and the layout rule (a plain apply's), every mrec_bwd_mode,
 * stochastic rounding, co-launched reductions, the same segment sums -- the result is
 * bitwise that of the plain entry over the expanded gradient.  bag_len >= 1, batch a
 * multiple of it, bag_scale non-NULL, dfm NULL (the FM term is undefined for bags).
 */
mrec_status mrec_emb_bwd_apply_bag(const mrec_table_bank *bank, int64_t batch,
                                   const void *workspace, size_t ws_bytes, const void *dx,
                                   mrec_dtype dx_dtype, int64_t dx_ld, const float *dfm,
                                   const float *fm_sum, const void *x0, mrec_dtype x0_dtype,
                                   int64_t x0_ld, const float *dw, mrec_bwd_mode mode, float lr,
                                   uint64_t seed, const uint64_t *d_step, void *grad,
                                   int32_t n_reduce, const struct mrec_gemm_call_s *reduce,
                                   mrec_stream stream, int32_t bag_len, const float *bag_scale);
mrec_status mrec_emb_bwd_large_fused_bag(const mrec_table_bank *bank, const mrec_ids *ids,
                                         int64_t batch, void *workspace, size_t ws_bytes,
                                         int32_t *d_oob_flag, const void *dx, mrec_dtype dx_dtype,
                                         int64_t dx_ld, const float *dfm, const float *fm_sum,
                                         const void *x0, mrec_dtype x0_dtype, int64_t x0_ld,
                                         const float *dw, mrec_bwd_mode mode, float lr,
                                         uint64_t seed, const uint64_t *d_step, void *grad,
                                         int32_t n_reduce, const struct mrec_gemm_call_s *reduce,
                                         mrec_stream stream, int32_t bag_len,
                                         const float *bag_scale);

/*
 * mrec_emb_bwd_apply with the per-lookup gradient rows given directly instead of
 * derived from dx / dfm / dw (those must be NULL when g_occ is set): lookup b of
 * table f contributes g_occ[idx * g_ld + 0 .. dim(+1)), idx = b when chunk == 0,
 * else (b / chunk) * chunk_stride + f * chunk + b % chunk — the receive buffer of
 * mrec_shard_lookup_grad rows after the reverse all-to-all (fp32, g_ld % 4 == 0).
 * The owner side of a row-sharded table (SURVEY.md §8e backward).  Like
 * mrec_emb_bwd_apply_ex, up to 6 deferred weight-gradient reductions may ride along.
 */
mrec_status mrec_emb_bwd_apply_given(const mrec_table_bank *bank, int64_t batch,
                                     const void *workspace, size_t ws_bytes, const void *dx,
                                     mrec_dtype dx_dtype, int64_t dx_ld, const float *dfm,
                                     const float *fm_sum, const void *x0, mrec_dtype x0_dtype,
                                     int64_t x0_ld, const float *dw, const float *g_occ,
                                     int64_t g_ld, int64_t chunk, int64_t chunk_stride,
                                     mrec_bwd_mode mode, float lr, uint64_t seed,
                                     const uint64_t *d_step, void *grad, int32_t n_reduce,
                                     const struct mrec_gemm_call_s *reduce, mrec_stream stream);
/* The owner's apply reading the received gradient RECORDS in place (ABI 23): no
 * unpack to fp32 slots.  Entry j of part p (exchange view: b = p * chunk + j,
 * chunk = cap, chunk_stride = the int32 per part of the ids message) of table f has
 * its gradient in record p * cap_rows + pref[p * n_tables + f] + j of `wire`
 * (rec_bytes each, wire_dtype BF16 or F32, 4-B aligned; pref from
 * mrec_shard_gather_wire_ex).  Same sums, order and update as mrec_emb_bwd_apply_given
 * on the unpacked slots (bit-identical). */
mrec_status mrec_emb_bwd_apply_wire(const mrec_table_bank *bank, int64_t batch,
                                    const void *workspace, size_t ws_bytes, const void *wire,
                                    int32_t rec_bytes, mrec_dtype wire_dtype, const int32_t *pref,
                                    int32_t cap_rows, int64_t chunk, int64_t chunk_stride,
                                    mrec_bwd_mode mode, float lr, uint64_t seed,
                                    const uint64_t *d_step, void *grad, int32_t n_reduce,
                                    const struct mrec_gemm_call_s *reduce, mrec_stream stream);
/* mrec_emb_bwd_apply_wire plus the data-parallel dense SGD of an
 * mrec_sgd_table_build table (device copy; sgd_blocks workgroups) in the same
 * launch (ABI 28) */
mrec_status mrec_emb_bwd_apply_wire_sgd(const mrec_table_bank *bank, int64_t batch,
                                        const void *workspace, size_t ws_bytes, const void *wire,
                                        int32_t rec_bytes, mrec_dtype wire_dtype,
                                        const int32_t *pref, int32_t cap_rows, int64_t chunk,
                                        int64_t chunk_stride, mrec_bwd_mode mode, float lr,
                                        uint64_t seed, const uint64_t *d_step, void *grad,
                                        int32_t n_reduce, const struct mrec_gemm_call_s *reduce,
                                        const void *sgd_table, int32_t sgd_blocks,
                                        mrec_stream stream);
/* The sender's DENSE_GRAD sums written straight as wire RECORDS (ABI 26): the
 * bank is the slot rows the interaction read (ids = pos, slot s = (p * n_tables +
 * f) * cap + j); slot s's sum goes to record p * cap_rows + pref[p * n_tables + f]
 * + j of `wire` (rec_bytes each, the table dtype, 4-B aligned; pref from
 * mrec_shard_wire_unpack_ex) -- the bytes mrec_shard_wire_pack would produce from
 * a zeroed sum buffer (bit-identical), without that buffer, its zeroing or the pack
 * launch.  Entries past a part's cap_rows are dropped (the unpack flagged them).
 * Hash layout only (batch <= MREC_BWD_HASH_MAX_BATCH). */
typedef struct {
  void *wire;
  int32_t rec_bytes;
  const int32_t *pref;
  int32_t cap;
  int32_t cap_rows;
} mrec_grad_records;
mrec_status mrec_emb_bwd_apply_rec(const mrec_table_bank *bank, int64_t batch,
                                   const void *workspace, size_t ws_bytes, const void *dx,
                                   mrec_dtype dx_dtype, int64_t dx_ld, const float *dfm,
                                   const float *fm_sum, const void *x0, mrec_dtype x0_dtype,
                                   int64_t x0_ld, const float *dw, const mrec_grad_records *out,
                                   int32_t n_reduce, const struct mrec_gemm_call_s *reduce,
                                   mrec_stream stream);

/* ------------------------------------------------------------------------- */
/* Communicator (RCCL over xGMI) for the row-sharded exchange                  */
/* ------------------------------------------------------------------------- */
/*
 * SURVEY.md §8(b) B2 comm entry points: with these and the mrec_shard_* kernels a
 * binding that is not torch (cgo, JNI, a C++ trainer) runs the sharded step.  The
 * reference has no communication at all (torchrec/task/Task.py:187-190 trains on
 * one device).  RCCL is opened at run time (MREC_RCCL_LIB, else the librccl
 * already in the process, else librccl.so): MREC_ERCCL when absent.
 *
 * Rank 0 calls mrec_comm_unique_id and hands the 128 bytes to every rank by any
 * host channel; each rank (one process per GPU, its HIP device current) calls
 * mrec_comm_init.  Exchanges are equal-split all-to-alls: part p of `send` (W
 * parts of the given size) goes to rank p, part p of `recv` comes from rank p --
 * the layout of mrec_shard_bucketize / mrec_shard_gather / mrec_shard_lookup_grad
 * buffers.  Stream-ordered on the caller's stream, capturable in a HIP graph; a
 * graph that captured them must be destroyed before mrec_comm_destroy (RCCL waits
 * for it).
 */
#define MREC_COMM_ID_BYTES 128
typedef struct mrec_comm_s mrec_comm;
mrec_status mrec_comm_unique_id(void *id_out /* MREC_COMM_ID_BYTES */);
mrec_status mrec_comm_init(const void *unique_id, int32_t rank, int32_t world, mrec_comm **out);
mrec_status mrec_comm_destroy(mrec_comm *comm);
int32_t mrec_comm_world(const mrec_comm *comm);
int32_t mrec_comm_rank(const mrec_comm *comm);
/* ids of the lookups for each owner: W x per_peer int32 (mrec_shard_bucketize send_ids) */
mrec_status mrec_a2a_ids(mrec_comm *comm, const int32_t *send_ids, int32_t *recv_ids,
                         int64_t per_peer, mrec_stream stream);
/* gathered rows back to the requesters: W x bytes_per_peer (multiple of 16) */
mrec_status mrec_a2a_rows_fwd(mrec_comm *comm, const void *send_rows, void *recv_rows,
                              int64_t bytes_per_peer, mrec_stream stream);
/* per-lookup gradient rows to the owners: W x floats_per_peer fp32 */
mrec_status mrec_a2a_rows_bwd(mrec_comm *comm, const float *send_grads, float *recv_grads,
                              int64_t floats_per_peer, mrec_stream stream);
/* the data-parallel dense gradient buffer, summed over the ranks in place */
mrec_status mrec_allreduce_sum_f32(mrec_comm *comm, float *buf, int64_t n, mrec_stream stream);

/* ------------------------------------------------------------------------- */
/* Row-sharded tables (one process per GPU, W = world size)                   */
/* ------------------------------------------------------------------------- */
/*
 * Table f is split cyclically: id i lives on rank i % W as local row i / W.  Every
 * exchange buffer has W equal parts of [n_tables][cap] slots (fixed capacity per
 * (owner, table)), so the all-to-alls are equal-split, need no host sync and can be
 * captured in a HIP graph.  Padding slots hold -1.  The reference has no sharding;
 * this replaces the dense nn.Embedding of IModel._init_weights (FunkSVD.py:39-41)
 * when a table does not fit, or should not be replicated on, one GPU.
 */

/*
 * Sender side, forward.  For each table f and sample b (ascending, stable):
 * owner = id % W, slot = rank of (b) among this table's ids with that owner;
 *   send_ids[(owner * n_tables + f) * cap + slot] = id / W
 *   pos[f * batch + b] = (owner * n_tables + f) * cap + slot
 * Unused slots get -1.  An id outside [0, rows[f]) sets *d_oob_flag and gets
 * pos = -1; a slot >= cap sets *d_overflow (the caller must raise) and pos = -1.
 * One 1024-thread workgroup per table; requires (W + 1) * ceil(batch/64) <= 2048.
 */
mrec_status mrec_shard_bucketize(const mrec_ids *ids, int32_t n_tables, const int64_t *rows,
                                 int64_t batch, int32_t world, int32_t cap, int32_t *send_ids,
                                 int32_t *pos, int32_t *d_overflow, int32_t *d_oob_flag,
                                 mrec_stream stream);

/*
 * Owner side, forward: rows_out[j, :] = local bank row of recv_ids[j] (table
 * f = (j / cap) % n_tables), whole row_stride elements, zeros for padding (-1) or
 * an out-of-shard id.  recv_ids / rows_out have world * n_tables * cap entries.
 */
mrec_status mrec_shard_gather(const mrec_table_bank *local, const int32_t *recv_ids,
                              int32_t world, int32_t cap, void *rows_out, mrec_stream stream);

/*
 * Sender side, backward: the gradient row of every lookup, written where its
 * embedding row came from (g_out[pos[f*batch+b] * g_ld + ...], fp32):
 *   g[d] = dx[b, f*dim + d] + dfm[b] * (fm_sum[b, d] - x0[b, f*dim + d]),  g[dim] = dw[b]
 * (same terms and NULL rules as mrec_emb_bwd_apply); lookups with pos < 0 skipped.
 */
mrec_status mrec_shard_lookup_grad(int64_t batch, int32_t n_tables, int32_t dim, int32_t has_w,
                                   const int32_t *pos, const void *dx, mrec_dtype dx_dtype,
                                   int64_t dx_ld, const float *dfm, const float *fm_sum,
                                   const void *x0, mrec_dtype x0_dtype, int64_t x0_ld,
                                   const float *dw, float *g_out, int64_t g_ld,
                                   mrec_stream stream);

/*
 * Compact exchange (ABI 19).  What crosses xGMI per step is one record per
 * DISTINCT (owner, table, id) each way instead of one 64-B slot row forward and
 * one fp32 slot row back per lookup:
 *   sender  mrec_shard_bucketize_dedup -> all-to-all ids (W parts of
 *           n_tables*cap + n_tables int32: slots, then the per-table counts)
 *   owner   mrec_shard_gather_wire     -> all-to-all rows (W parts of cap_rows
 *           records of mrec_shard_wire_bytes each: bf16 dim 16 + w = 36 B)
 *   sender  mrec_shard_wire_unpack     -> rows in the slot layout of
 *           mrec_shard_gather (the interaction reads them by pos, unchanged)
 *   backward: the sender sums the gradients of the lookups of each slot (a
 *           DENSE_GRAD apply over the slot rows, fixed ascending order), packs them
 *           (mrec_shard_wire_pack, table dtype) -> all-to-all -> the owner unpacks
 *           them to fp32 slots (mrec_shard_wire_unpack, to_f32) for
 *           mrec_emb_bwd_apply_given.
 * A part's records: table f's entries at [prefix(f), prefix(f) + count(f)) with
 * prefix(f) = sum of the counts of tables < f, so cap_rows bounds the owner's
 * total over all tables (far tighter than n_tables * cap); more sets *d_overflow
 * (the caller raises; nothing is silently dropped from a valid step).
 */
mrec_status mrec_shard_bucketize_dedup(const mrec_ids *ids, int32_t n_tables, const int64_t *rows,
                                       int64_t batch, int32_t world, int32_t cap,
                                       int32_t *send_ids, int32_t *pos, int32_t *d_overflow,
                                       int32_t *d_oob_flag, mrec_stream stream);
/*
 * Batches past one workgroup's hash (ABI 25): the sender's batch is cut into
 * C = ceil(batch / chunk_batch) chunks (chunk_batch <= 8192), each its own
 * sub-sender -- part d * C + c of send_ids holds chunk c's distinct ids for owner d
 * (owner d's C parts contiguous, so the equal-split all-to-all moves W parts of
 * C * (n_tables*cap + n_tables) int32), pos addresses slot rows of W * C parts, and
 * every other compact-exchange call takes world = W * C.  An id repeated across
 * chunks takes a slot in each; the owner sums its entries in part order.
 */
mrec_status mrec_shard_bucketize_dedup_ex(const mrec_ids *ids, int32_t n_tables,
                                          const int64_t *rows, int64_t batch, int32_t world,
                                          int32_t cap, int64_t chunk_batch, int32_t *send_ids,
                                          int32_t *pos, int32_t *d_overflow, int32_t *d_oob_flag,
                                          mrec_stream stream);

/*
 * mrec_shard_bucketize_dedup_ex with `quarters` (a power of two <= 16) workgroups per
 * table and chunk (ABI 28): workgroup q takes the ids whose quarter
 * ((id * 0x9e3779b1) mod 2^32) >> (32 - log2 quarters) is q, so each inserts and
 * ranks a quarter of the distinct ids; a part's slots are quarter-major (quarter 0's
 * distinct ids in first-lookup order, then quarter 1's, ...) -- the same records and
 * sums, another slot order.  The quarters of a (table, chunk) meet once through
 * `scratch` (mrec_shard_dedup_scratch_bytes, zeroed once before first use, then kept
 * with the caller: it holds monotonic arrival tickets); a wait that times out sets bit
 * 2 of *d_overflow.  quarters = 1 is mrec_shard_bucketize_dedup_ex.
 */
size_t mrec_shard_dedup_scratch_bytes(int32_t n_tables, int64_t chunks, int32_t world,
                                      int32_t quarters);
mrec_status mrec_shard_bucketize_dedup_q(const mrec_ids *ids, int32_t n_tables,
                                         const int64_t *rows, int64_t batch, int32_t world,
                                         int32_t cap, int64_t chunk_batch, int32_t quarters,
                                         void *scratch, size_t scratch_bytes, int32_t *send_ids,
                                         int32_t *pos, int32_t *d_overflow, int32_t *d_oob_flag,
                                         mrec_stream stream);
/* bytes of one wire record: round4((dim + has_w) * element bytes) */
int32_t mrec_shard_wire_bytes(int32_t dim, int32_t has_w, mrec_dtype dtype);
/* owner: rows of the received ids (header = recv_ids) -> wire (a lazy-Adam bank's
 * rows caught up to the current step, ABI 25); 
 * plan (may be NULL, ABI 21): the owner's backward hash plan over the same received
 * ids (an exchange view, mrec_plan_job) run by leading workgroups of this launch */
mrec_status mrec_shard_gather_wire(const mrec_table_bank *local, const int32_t *recv_ids,
                                   int32_t world, int32_t cap, int32_t cap_rows, void *wire,
                                   int32_t *d_overflow, const mrec_plan_job *plan,
                                   mrec_stream stream);
/* the same, also writing pref [world][n_tables] int32: part p's table prefixes (record
 * of entry j of table f in part p = p * cap_rows + pref[p][f] + j).  The gradient
 * records the senders return have the layout of the ids they sent, so pref also
 * addresses them for mrec_emb_bwd_apply_wire (ABI 23) */
mrec_status mrec_shard_gather_wire_ex(const mrec_table_bank *local, const int32_t *recv_ids,
                                      int32_t world, int32_t cap, int32_t cap_rows, void *wire,
                                      int32_t *pref, int32_t *d_overflow,
                                      const mrec_plan_job *plan, mrec_stream stream);
/* wire records -> slot rows [(p * n_tables + f) * cap + j] (pitch slot_bytes; to_f32:
 * bf16 records widened to fp32); zero (may be NULL): zero_bytes of the same rows of a
 * second buffer are cleared (the sender's gradient sums) */
mrec_status mrec_shard_wire_unpack(const void *wire, int32_t rec_bytes, const int32_t *hdr_ids,
                                   int32_t world, int32_t n_tables, int32_t cap, int32_t cap_rows,
                                   void *slots, int64_t slot_bytes, int32_t to_f32, void *zero,
                                   int64_t zero_bytes, int32_t *d_overflow, mrec_stream stream);
/* the same, also writing pref [world][n_tables] int32 (may be NULL, ABI 26): part
 * p's table prefixes of hdr_ids' counts -- the sender's own record layout, which
 * mrec_emb_bwd_apply_rec writes the gradient records in */
mrec_status mrec_shard_wire_unpack_ex(const void *wire, int32_t rec_bytes, const int32_t *hdr_ids,
                                      int32_t world, int32_t n_tables, int32_t cap,
                                      int32_t cap_rows, void *slots, int64_t slot_bytes,
                                      int32_t to_f32, void *zero, int64_t zero_bytes,
                                      int32_t *pref, int32_t *d_overflow, mrec_stream stream);
/* slot rows -> wire records (the first rec_bytes of each row) */
mrec_status mrec_shard_wire_pack(const void *slots, int64_t slot_bytes, int32_t rec_bytes,
                                 const int32_t *hdr_ids, int32_t world, int32_t n_tables,
                                 int32_t cap, int32_t cap_rows, void *wire, int32_t *d_overflow,
                                 mrec_stream stream);

/* ------------------------------------------------------------------------- */
/* Dense towers: MFMA bf16 GEMM with fused epilogues                          */
/* ------------------------------------------------------------------------- */

typedef enum {
  MREC_LAYOUT_ROW = 0, /* element (i, k) at ptr[i*ld + k]  (k contiguous)   */
  MREC_LAYOUT_COL = 1  /* element (i, k) at ptr[k*ld + i]  (i contiguous)   */
} mrec_layout;

typedef struct {
  const void *ptr; /* device */
  mrec_dtype dtype;
  mrec_layout layout;
  int64_t ld; /* elements */
} mrec_operand;

#define MREC_ACT_NONE 0
#define MREC_ACT_RELU 1

#define MREC_IMG_ROW_TR 0 /* bf16 weight images: row-major [N, ld] and W^T [K, ld] */
#define MREC_IMG_TOWER 1  /* MFMA-fragment images of the fused tower (mrec_tower_*) */

/* v = acc + bias[n]; aux[m,n] = v; v = act(v); v *= mul[m,n]; v += add[m,n];
 * v = (mask[m,n] > 0) ? v : 0; C = v.  Every pointer may be NULL (term skipped);
 * mul/add/aux/mask are bf16 [M, ld].  `mask` applies the ReLU' of the layer that
 * produced this GEMM's *output* operand, so a backward GEMM emits the next
 * layer's pre-activation gradient directly.  With b_ones_col the extra column (the
 * row sums of A) goes to ones_out (fp32 [M]). */
typedef struct {
  const float *bias;
  int32_t act;
  const void *mul;
  int64_t ld_mul;
  const void *add;
  int64_t ld_add;
  void *aux;
  int64_t ld_aux;
  const void *mask;
  int64_t ld_mask;
  float *ones_out;
  /* Fused SGD (update != 0; then bias/act/mul/add/aux/mask must be unset and C
   * fp32): C is a master weight updated in place, C[m, n] -= lr * v, and
   * ones_out[m] -= lr * (row sum), instead of being overwritten; the new C is
   * re-emitted as bf16 images for the next forward, img_row[m * ld_img_row + n]
   * and img_tr[n * ld_img_tr + m] (either may be NULL).  A Linear's weight-gradient
   * GEMM then IS its torch.optim.SGD step (no momentum / weight decay;
   * IModel.py:116-125) — no gradient tensor, no optimizer or conversion kernels. */
  int32_t update;
  float lr;
  void *img_row;
  int64_t ld_img_row;
  void *img_tr;
  int64_t ld_img_tr;
  /* MREC_IMG_ROW_TR: img_row / img_tr as above; MREC_IMG_TOWER: they are the
   * fwd / bwd MFMA-fragment images of mrec_tower_fwd_bwd (ld_* ignored). */
  int32_t img_kind;
} mrec_epilogue;

size_t mrec_gemm_workspace_size(int64_t M, int64_t N, int64_t K, int32_t split_k);

/*
 * C[M, N] = epi( sum_k A(m, k) B(k, n) ), A and B bf16 with 16-byte aligned rows
 * (fp32 weights go through mrec_weight_prep), fp32 accumulation on
 * v_mfma_f32_16x16x32_bf16.  Each 256-thread workgroup computes a 64x64 tile over a
 * K slice; operands are brought into LDS by global_load_lds_dwordx4 (LDS-DMA,
 * swizzled images, no register staging) through a 3-deep ring of 64-wide k
 * groups, COL operands are read back with ds_read_b64_tr_b16; K is split over
 * split_k workgroups, partials reduced in fixed order (deterministic) through
 * `workspace` (mrec_gemm_workspace_size bytes).
 * Layout ROW: element (i, k) at ptr[i*ld + k]; COL: at ptr[k*ld + i] (for B, i is
 * the output column n; nn.Linear's [out, in] weight is B in ROW layout).
 * b_ones_col == N appends a column of ones to B, so epi->ones_out[m] = sum_k A(m, k):
 * the bias gradient of a weight-gradient GEMM.  B(k, n) = 0 for b_cols <= n < N.
 * Operand pad elements between K (or the valid rows) and the next multiple of 8 must
 * be zero; C's pad columns up to min(ldc, round8(N)) are written as zero.
 * Replaces nn.Linear forward/backward = aten::addmm / mm and the ReLU
 * (Dense.py:20-24, MLP.py:22-23; SURVEY.md §2b MLP row).
 */
mrec_status mrec_gemm(int64_t M, int64_t N, int64_t K, const mrec_operand *A,
                      const mrec_operand *B, int64_t b_ones_col, int64_t b_cols,
                      const mrec_epilogue *epi, void *C, mrec_dtype c_dtype, int64_t ldc,
                      int32_t split_k, void *workspace, size_t ws_bytes, mrec_stream stream);

/* phases of a GEMM inside mrec_gemm_multi */
#define MREC_GEMM_FULL 0    /* product + epilogue (split_k must resolve to 1) */
#define MREC_GEMM_PARTIAL 1 /* split-K: fp32 partial slabs into workspace only */
#define MREC_GEMM_REDUCE 2  /* split-K: fixed-order slab reduction + epilogue only */

typedef struct mrec_gemm_call_s {
  int64_t M, N, K;
  const mrec_operand *A;
  const mrec_operand *B;
  int64_t b_ones_col;
  int64_t b_cols;
  const mrec_epilogue *epi;
  void *C;
  mrec_dtype c_dtype;
  int64_t ldc;
  int32_t split_k;
  void *workspace;
  size_t ws_bytes;
  int32_t phase; /* MREC_GEMM_* */
} mrec_gemm_call;

/*
 * Up to 4 independent GEMM phases in ONE launch (same arguments and results as
 * mrec_gemm; a split-K GEMM is run as PARTIAL in one call and REDUCE in a later one,
 * same arguments and workspace).  The calls must not depend on each other.  Used
 * for a backward layer: its dx GEMM, its dW partial slabs and the previous layer's
 * dW reduction (+ fused SGD) overlap instead of paying three launch boundaries.
 */
mrec_status mrec_gemm_multi(int32_t n, const mrec_gemm_call *calls, mrec_stream stream);



/* the CTR head's parameter finish (arguments of mrec_ctr_head_finish) */
typedef struct {
  const float *part;
  int64_t ldp;
  int64_t batch;
  int32_t H, ns;
  const float *g;
  int32_t update;
  float lr;
  float *w, *bias, *ws, *b2;
  float *dw_out, *db_out, *dws_out, *db2_out;
} mrec_head_finish_job;

/*
 * mrec_gemm_multi plus, in extra workgroups of the same launch, the CTR head
 * finish of `finish` (may be NULL).  A HIP graph runs the step's kernels one
 * after another, so a small kernel of its own sits on the critical path; beside
 * latency-bound backward GEMMs it is hidden.  Same results as
 * mrec_ctr_head_finish.  The job must be independent of the GEMM calls.
 * `plan` must be NULL (ABI 12): the embedding-backward plan rides in the
 * interaction launch (mrec_interact_fwd_ex) -- inside a GEMM launch its
 * registers held the GEMM at half occupancy -- and a plan job here is EINVAL.
 */
mrec_status mrec_gemm_multi_ex(int32_t n, const mrec_gemm_call *calls, const mrec_plan_job *plan,
                               const mrec_head_finish_job *finish, mrec_stream stream);

/*
 * fp32 [N, K] weight (row stride ldw) -> bf16 images for the GEMMs: `row`
 * [N, ldr] (B operand of the forward) and/or `tr` = W^T [K, ldt] (B operand of the
 * input-gradient GEMM); pad columns are zero.  One launch per weight per step
 * keeps the fp32 master weights as the optimizer's parameters.
 */
mrec_status mrec_weight_prep(const float *W, int64_t N, int64_t K, int64_t ldw, void *row,
                             int64_t ldr, void *tr, int64_t ldt, mrec_stream stream);

/*
 * DCN-v2 cross-network backward, elementwise stage of layer l (bf16 [M, d] rows,
 * SURVEY.md §8(a) A10): dz = g*x0; acc = (acc_init ? 0 : acc) + g*z (fp32); if
 * addend != NULL, addend = bf16(acc + g) (layer 0: its dx_l GEMM adds it and
 * yields dx0).  All rows hold round8(d) columns, 16-byte aligned; pad columns of
 * dz / acc / addend are zeroed.
 */
mrec_status mrec_dcn_cross_bwd_prep(int64_t M, int64_t d, const void *g, int64_t ldg,
                                    const void *x0, int64_t ldx0, const void *z, int64_t ldz,
                                    void *dz, int64_t lddz, float *acc, int64_t ldacc,
                                    int32_t acc_init, void *addend, int64_t ldadd,
                                    mrec_stream stream);

/*
 * Data-parallel dense update: for each job, w -= lr * g over an fp32 [N, K]
 * parameter (row strides ldw / ldg; a vector is N = 1), then the weight's bf16
 * images are re-emitted from the new w like mrec_weight_prep (`img_row` [N, ld_row]
 * and/or `img_tr` = W^T [K, ld_tr], pad columns zero; either may be NULL).  Up to
 * 16 jobs, ONE launch.  Replaces torch.optim.SGD.step() on the all-reduced
 * gradients (optimizers.py:7-11, reached from IModel.train_step, IModel.py:122-124)
 * plus a weight_prep per layer; lr already carries the 1/world of the gradient mean.
 */
typedef struct {
  float *w;
  const float *g;
  int64_t N, K, ldw, ldg;
  float lr;
  void *img_row;
  int64_t ld_row;
  void *img_tr;
  int64_t ld_tr;
  int32_t img_kind; /* MREC_IMG_ROW_TR or MREC_IMG_TOWER (see mrec_epilogue) */
} mrec_sgd_job;

mrec_status mrec_sgd_multi(int32_t n, const mrec_sgd_job *jobs, mrec_stream stream);

/*
 * The same jobs as a table another launch runs (ABI 28): mrec_sgd_table_build
 * validates them and writes the table (mrec_sgd_table_bytes() bytes, host memory)
 * and its workgroup count; the caller copies it to a 16-B aligned device buffer once
 * (it holds pointers and lr, not data) and passes that to
 * mrec_emb_bwd_apply_wire_sgd, which runs the SGD tiles beside the owner's
 * embedding update -- after the flat gradient's all-reduce, instead of a
 * mrec_sgd_multi launch of its own.  Same arithmetic, same bits.
 */
size_t mrec_sgd_table_bytes(void);
mrec_status mrec_sgd_table_build(int32_t n, const mrec_sgd_job *jobs, void *out, size_t out_bytes,
                                 int32_t *blocks);

/*
 * Fused MLP tower + CTR head + BCE loss, forward AND the input-gradient half of
 * the backward, in ONE launch (the reference's MLP =
 * Linear -> ReLU per layer (MLP.py:8-23, Dense.py:4-24), then Linear(N_L, 1) and
 * the loss of IModel.train_step (IModel.py:116-125)).  Every row of the batch is
 * independent until the weight gradients, so one 512-thread workgroup owns 16 rows
 * for the whole chain: activations stay in LDS, the bf16 weights stream from L2
 * in MFMA-fragment order (v_mfma_f32_16x16x32_bf16, fp32 accumulation), and
 *   h_l = relu(h_{l-1} W_l^T + b_l), l = 1..L (h_0 = x0);
 *   z = h_L . head_w + head_b + base + xs . ws + b2;  loss = mean BCE(z, y);
 *   dz = (sigmoid(z) - y) / batch;  dh_L = dz head_w * [h_L > 0];
 *   dh_{l-1} = (dh_l W_l) * [h_{l-1} > 0];  dx0 = dh_1 W_1.
 * Outputs (bf16 [batch, ld], pad columns zero): h_out[l] for l < L (NULL: not
 * stored), dh_out[l] for every l (the weight-gradient GEMMs' operands), dx0
 * (NULL: not stored); fp32 z, dz [batch]; the head-parameter partials (one row of
 * [dW_head (N_L) | sum dz | dws (ns)] per 16 rows, the layout
 * mrec_ctr_head_finish reduces; ceil(batch/16) rows); the loss (ticket / last
 * workgroup, deterministic, like mrec_ctr_head_fwd).
 * Weights: w_fwd[l] / w_bwd[l] are the layer's tower images (mrec_tower_weight_prep;
 * the fused SGD epilogues keep them current with img_kind = MREC_IMG_TOWER).
 * Limits: 1 <= L <= 4, every width in [1, 512], ns <= 64.
 */
typedef struct {
  int64_t batch;
  int32_t n_layers;
  int32_t width[5];          /* width[0] = x0 columns (K0), width[l] = N_l */
  const void *x0;            /* bf16 [batch, ld_x0], ld_x0 >= round8(K0), pad columns zero */
  int64_t ld_x0;
  const void *w_fwd[4];      /* bf16 tower images of W_l [N_l, N_{l-1}] */
  const void *w_bwd[4];
  const float *bias[4];      /* [N_l] (NULL: no bias) */
  const float *head_w;       /* [N_L] */
  const float *head_b;       /* [1] or NULL */
  const float *base;         /* [batch] per-sample logit added to z (FM part) or NULL */
  const float *xs;           /* side linear: xs [batch, ld_xs] fp32 . ws [ns] (+ b2) */
  int64_t ld_xs;
  int32_t ns;
  const float *ws;
  const float *b2;
  const float *y;            /* labels [batch] */
  void *h_out[4];
  int64_t ld_h[4];
  void *dh_out[4];
  int64_t ld_dh[4];
  void *dx0;
  int64_t ld_dx0;
  float *z;                  /* may be NULL */
  float *dz;
  float *part;
  int64_t ldp;               /* >= N_L + 1 + ns */
  float *loss_part;          /* [ceil(batch/16)] scratch */
  uint32_t *ticket;          /* device word, zero before the first call; left zero */
  float *loss;               /* [1] */
  /* ABI 15: kfrag != 0 -> h_out[l] / dh_out[l] are k-fragment images of [batch,
   * N_l] (mrec_kfrag_elems; ld_h / ld_dh ignored) and x0_img (may be NULL) receives
   * the k-fragment image of x0 [batch, N_0]: the operands of mrec_tower_dw */
  int32_t kfrag;
  void *x0_img;
  /* ABI 16: what runs after the forward (MREC_TOWER_*).  BCE: the loss above.
   * FORWARD: z only (h_L . head_w + head_b + base + xs . ws + b2, z required), then
   * the launch ends (no y, dz, part, loss, stores; the attention unit's scores).
   * GIVEN_DZ: dz = dz_in (no loss; y, loss_part, ticket, loss, dz may be NULL); the
   * backward as for BCE (dh_out, dx0, head partials, images). */
  int32_t mode;
  const float *dz_in;        /* [batch] for MREC_TOWER_GIVEN_DZ */
  /* ABI 27: a DCN-v2 cross network ahead of the MLP (the
   * layers are nn.Linear(d, d) as the reference's Linear init, IModel.py:61-66),
   * n_cross layers of width d = width[0], run in the same launch on the x0 block:
   *   x_0 = x0;  z_c = x_c Wc_c^T + bc_c;  x_{c+1} = x0 * z_c + x_c;  the MLP reads
   *   x_{n_cross} (its h_0);
   * backward (G_{n_cross} = the MLP's input gradient):
   *   dz_c = G_{c+1} * x0;  G_c = dz_c Wc_c + G_{c+1};
   *   dx0 = G_0 + sum_c G_{c+1} * z_c   (fp32 sum, one rounding, written to dx0).
   * With kfrag: x0_img receives x_0's image, cross_x_img[c] the image of x_{c+1}
   * (cross_x_img[n_cross - 1] is the MLP's first-layer X operand) and
   * cross_dz_img[c] that of dz_c: with them mrec_tower_dw computes dWc_c =
   * dz_c^T [x_c | 1].  z_c stays on chip (bf16) from the forward to the backward. */
  int32_t n_cross;           /* 0..3 */
  const void *cross_w_fwd[3];  /* tower images of Wc_c [d, d] */
  const void *cross_w_bwd[3];
  const float *cross_bias[3];  /* [d] (NULL: no bias) */
  void *cross_x_img[3];
  void *cross_dz_img[3];
} mrec_tower_args;

enum { MREC_TOWER_BCE = 0, MREC_TOWER_FORWARD = 1, MREC_TOWER_GIVEN_DZ = 2 };

mrec_status mrec_tower_fwd_bwd(const mrec_tower_args *a, mrec_stream stream);

/*
 * Weight gradients of the fused tower (ABI 15): for every layer l,
 *   partial slab z of dW_l [n_out, n_in + 1] = sum over K slice z of the batch of
 *   dY_l[b]^T [X_l[b] | 1]        (column n_in: the bias gradient)
 * written to ws[l] + z * n_out * ldws[l] (fp32) -- exactly the split-K PARTIAL slabs
 * of mrec_gemm(n_out, n_in, batch, dY_l COL, X_l COL, b_ones_col = n_in, ...,
 * split_k = splits), so a later mrec_gemm_multi REDUCE job of that call (same
 * workspace) finishes it (fixed-order sum + epilogue / fused SGD).  `splits` must
 * be an effective count for the batch (B = 4096: 2, 4, 5, 8, 16 ...).
 * dy_img / x_img are k-fragment images (mrec_kfrag_elems / mrec_kfrag_pack; the
 * tower writes them, mrec_tower_args.kfrag).  `finish` (may be NULL): the CTR head
 * finish in extra workgroups of the same launch (as mrec_gemm_multi_ex).
 * Replaces the weight-gradient half of autograd through nn.Linear in the
 * reference MLP (MLP.py:8-23, Dense.py:12-24) for the tower path.
 */
typedef struct {
  int32_t n_layers;          /* 1..8 (ABI 27: 8, the cross layers + the MLP) */
  int64_t batch;
  int32_t n_out[8], n_in[8];
  const void *dy_img[8];     /* bf16 k-fragment image of dY_l [batch, n_out] */
  const void *x_img[8];      /* bf16 k-fragment image of X_l [batch, n_in] */
  float *ws[8];              /* splits x n_out x ldws fp32 */
  int64_t ldws[8];           /* >= n_in + 1 (mrec_gemm's slab stride: round8(n_in + 1)) */
  int32_t splits;
} mrec_tower_dw_args;

mrec_status mrec_tower_dw(const mrec_tower_dw_args *args, const mrec_head_finish_job *finish,
                          mrec_stream stream);
/* ABI 27: + the batch feed's copy of the next record in extra workgroups (feed may be
 * NULL; see mrec_feed_job) */
struct mrec_feed_job_s; /* mrec_feed_job, defined with the batch feed below */
mrec_status mrec_tower_dw_ex(const mrec_tower_dw_args *args, const mrec_head_finish_job *finish,
                             const struct mrec_feed_job_s *feed, mrec_stream stream);

/* elements of the k-fragment image of a [rows, cols] matrix: one 1 KiB block per 16
 * columns x 32 rows, block (c / 16) * ceil(rows / 32) + r / 32, lane
 * c % 16 + 16 ((r % 32) / 8), element r % 8 (the MFMA operand order) */
int64_t mrec_kfrag_elems(int64_t rows, int64_t cols);

/* row-major bf16 [rows, cols] (row stride ld) -> its k-fragment image (pads zero) */
mrec_status mrec_kfrag_pack(const void *x, int64_t rows, int64_t cols, int64_t ld, void *img,
                            mrec_stream stream);

/* elements of the fwd (bwd = 0) or bwd (bwd = 1) tower image of an [N, K] weight */
int64_t mrec_tower_image_elems(int64_t N, int64_t K, int32_t bwd);

/* fp32 W [N, K] (row stride ldw) -> its tower images (either may be NULL).  Only
 * real elements are written: allocate the images zeroed once. */
mrec_status mrec_tower_weight_prep(const float *W, int64_t N, int64_t K, int64_t ldw,
                                   void *img_fwd, void *img_bwd, mrec_stream stream);

/* ------------------------------------------------------------------------- */
/* Batch feed                                                                 */
/* ------------------------------------------------------------------------- */

/* Copy one packed batch record (pytorchrec_amd/loader.py PackedLayout) from
 * PINNED, device-visible host memory into its device slot with a kernel on
 * `stream` (the compute queue reads the host pages over PCIe; no DMA engine, so
 * a graph launched behind it does not wait on the host).  16-B aligned, bytes a
 * multiple of 16.  Replaces the per-tensor blocking `.to(device)` of
 * IModel.train_step (torchrec/model/IModel.py:119) fed by
 * SimpleDataReader.__getitem__ (torchrec/data/SimpleDataReader.py:323-331). */
mrec_status mrec_batch_stage(void *dst, const void *host_src, int64_t bytes, mrec_stream stream);

/* ABI 27: the record at a DEVICE cursor of a pinned epoch buffer (n_records records
 * of record_bytes each, one pinned allocation): copies record d_state[0] (nothing
 * when it is past the last) into dst, then advances d_state[0] by one (d_state[1]:
 * a ticket word, zero before the first call, left zero).  Captured into a HIP graph
 * on a branch beside the train step, every replay stages the next batch while the
 * step runs (no host work per step; loader.py ColumnarLoader.capture_steps). */
mrec_status mrec_batch_stage_cursor(void *dst, const void *host_base, int64_t record_bytes,
                                    int64_t n_records, uint64_t *d_state, mrec_stream stream);

/* The same copy as a job another launch runs in extra workgroups (ABI 27:
 * mrec_tower_dw_ex), so the PCIe reads overlap that launch's work instead of taking
 * their own ~15 us on the step's critical path. */
typedef struct mrec_feed_job_s {
  void *dst;                 /* the device slot (16-B aligned) */
  const void *host_base;     /* the pinned epoch buffer: n_records x record_bytes */
  int64_t record_bytes;
  int64_t n_records;
  uint64_t *d_state;         /* [0] cursor (the record to copy, advanced by one), [1] ticket */
  /* ABI 29: the record's first widen_bytes (a multiple of 16) hold uint16 values the
   * copy writes as int32 (zero-extended): the device slot is record_bytes +
   * widen_bytes long, the rest of the record lands after the widened prefix.  The
   * loader packs ids below 65,536 this way (a third less PCIe per C2 batch); 0: a
   * plain copy */
  int64_t widen_bytes;
} mrec_feed_job;

/* ABI 29: mrec_batch_stage with a widened uint16 prefix (see mrec_feed_job) */
mrec_status mrec_batch_stage_ex(void *dst, const void *host_src, int64_t bytes, int64_t widen_bytes,
                                mrec_stream stream);
/* ABI 29: a feed job as a launch of its own (mrec_batch_stage_cursor with the job's
 * widened prefix) */
mrec_status mrec_batch_stage_job(const mrec_feed_job *job, mrec_stream stream);

/* ------------------------------------------------------------------------- */
/* CTR head and loss                                                          */
/* ------------------------------------------------------------------------- */

/*
 * z[b] = base[b] + bias[0] + h[b, :H] . w   (h bf16 rows, 16-B aligned; w fp32 [H];
 * base/bias may be NULL).  The deep tower's Linear(H, 1) (NCF.py:51, 74) fused
 * with the sum of the wide/FM logit.
 */
mrec_status mrec_head_fwd(const void *h, int64_t ldh, int64_t batch, int32_t H, const float *w,
                          const float *bias, const float *base, float *z, mrec_stream stream);
/* dh[b, :] = dz[b] * w  (bf16, pad columns up to ldh zeroed); with `mask` (bf16
 * [batch, ld_mask], may be NULL) dh[b, h] = 0 where mask[b, h] <= 0: the ReLU' of
 * the layer that produced h, so dh is that layer's pre-activation gradient. */
mrec_status mrec_head_bwd(const float *dz, const float *w, int64_t batch, int32_t H,
                          const void *mask, int64_t ld_mask, void *dh, int64_t ldh,
                          mrec_stream stream);

/*
 * torch.nn.BCEWithLogitsLoss (mean): *loss = mean(max(z,0) - z y + log1p(exp(-|z|)))
 * (fixed-order reduction); backward dz = g[0] (sigmoid(z) - y) / B (g may be NULL = 1).
 * The CTR loss the reference lacks (losses.py:8-12 has BPR/Top1/MSE only).
 */
mrec_status mrec_bce_fwd(const float *z, const float *y, int64_t batch, float *loss,
                         mrec_stream stream);
mrec_status mrec_bce_bwd(const float *z, const float *y, int64_t batch, const float *g, float *dz,
                         mrec_stream stream);

/* ------------------------------------------------------------------------- */
/* DIN target attention (config C4; absent from the reference: SURVEY.md A11) */
/* ------------------------------------------------------------------------- */
/*
 * feat[b*L + j, :] = [q_b | k_bj | q_b - k_bj | q_b * k_bj]   (bf16, 4E columns)
 * — the attention-unit input; q [B, E], k [B*L, E] bf16 (the gathered target and
 * history rows), 16-B aligned rows, E % 8 == 0, E <= 64, L <= 64.
 */
mrec_status mrec_din_feat_fwd(const void *q, int64_t ldq, const void *k, int64_t ldk,
                              int64_t batch, int32_t L, int32_t E, void *feat, int64_t ldf,
                              mrec_stream stream);
/*
 * Masked softmax pooling, one wave per sample: a_bj = softmax_j(s_bj) over valid j
 * (his[b, j] > 0 or j == 0: get_valid_his_index, torchrec/model/utils.py:5-10;
 * invalid -> -inf as scaled_dot_product_attention, SASRec.py:26-29);
 * top[b, :] = [q_b | sum_j a_bj k_bj | 0-pad] (bf16, the top MLP's input).
 * s[(b*L + j) * ld_s] fp32 scores; a [B, L] fp32 saved for the backward.
 */
mrec_status mrec_din_pool_fwd(const float *s, int64_t ld_s, const int32_t *his, int64_t ld_his,
                              const void *q, int64_t ldq, const void *k, int64_t ldk,
                              int64_t batch, int32_t L, int32_t E, float *a, void *top,
                              int64_t ldt, mrec_stream stream);
/* pooling backward from dtop[:, E:2E] = du: ds_bj = a_bj (du.k_bj - sum_i a_bi du.k_bi),
 * dk_bj = a_bj du (fp32, written) */
mrec_status mrec_din_pool_bwd(const void *dtop, int64_t lddt, const float *a, const void *k,
                              int64_t ldk, int64_t batch, int32_t L, int32_t E, float *ds,
                              float *dk, int64_t lddk, mrec_stream stream);
/* attention-unit input backward: dk_bj += df_k - df_(q-k) + df_(q*k) q_b;
 * dq_b = dtop[b, :E] + sum_j (df_q + df_(q-k) + df_(q*k) k_bj)  (position order) */
mrec_status mrec_din_feat_bwd(const void *dfeat, int64_t lddf, const void *dtop, int64_t lddt,
                              const void *q, int64_t ldq, const void *k, int64_t ldk,
                              int64_t batch, int32_t L, int32_t E, float *dk, int64_t lddk,
                              float *dq, int64_t lddq, mrec_stream stream);
/* the same, with dq and the final dk written as ONE bf16 gradient of the gathered
 * rows [target rows b < batch | history rows batch + b L + j] (row stride ld_rows;
 * dk read, not written): the gather's input gradient in the bank's dtype (ABI 15) */
mrec_status mrec_din_feat_bwd_rows(const void *dfeat, int64_t lddf, const void *dtop, int64_t lddt,
                                   const void *q, int64_t ldq, const void *k, int64_t ldk,
                                   int64_t batch, int32_t L, int32_t E, const float *dk,
                                   int64_t lddk, void *d_rows, int64_t ld_rows, mrec_stream stream);

/*
 * DIN lookup ids (ABI 17): out_item / out_cate [batch + batch L] int32 =
 * [target ids | history ids with PAD positions (his == 0 and j > 0) as -1].
 * Any other id that is negative or >= 2^31 (a target, position 0, a negative his,
 * the category of a non-PAD position) is written as INT32_MAX so that the gather's
 * range check reports it (tables must have < 2^31 - 1 rows), as nn.Embedding raises
 * IndexError on it (the reference models under torchrec/model/).
 * With mrec_ids.pad_negative set, the gather returns a zero row for -1 and the
 * embedding backward skips it: a masked history position has an exactly zero
 * gradient (softmax weight 0), so its PAD-row lookups need no update.
 * iid / cid [batch], his / hcat [batch, ld >= L], all of ids_dtype (I32 / I64).
 */
mrec_status mrec_din_lookup_ids(const void *iid, const void *cid, const void *his, int64_t ld_his,
                                const void *hcat, int64_t ld_hcat, int32_t ids_dtype,
                                int64_t batch, int32_t L, int32_t *out_item, int32_t *out_cate,
                                mrec_stream stream);

/*
 * mrec_din_lookup_ids and mrec_emb_gather_fwd (pad_negative) in ONE launch (ABI 22):
 * writes the same out_item / out_cate ids (for the embedding backward) and gathers
 * the rows of both tables into out [batch (L + 1), 2 dim] (item | category; a
 * padding slot is a zero row).  bank: the two tables (item, category), not under
 * the lazy fused Adam.  An invalid id sets *d_oob_flag (the caller raises
 * IndexError, as for nn.Embedding).  Replaces, with the ids builder, the
 * reference's nn.Embedding lookups of target and history ids (SASRec.py:85-86 idiom;
 * torchrec has no DIN).
 */
mrec_status mrec_din_gather(const mrec_table_bank *bank, const void *iid, const void *cid,
                            const void *his, int64_t ld_his, const void *hcat, int64_t ld_hcat,
                            int32_t ids_dtype, int64_t batch, int32_t L, int32_t *out_item,
                            int32_t *out_cate, void *out, mrec_dtype out_dtype, int64_t out_ld,
                            int32_t *d_oob_flag, mrec_stream stream);

/*
 * Fused DIN attention unit (ABI 17): one launch each way replaces
 * mrec_din_feat_fwd + the attention MLP's GEMMs + Linear(H2, 1) + mrec_din_pool_fwd
 * (forward) and mrec_din_pool_bwd + the GEMMs' backward + mrec_din_feat_bwd_rows
 * (backward).  Per sample, in LDS only: X = [q | k_j | q - k_j | q * k_j] (bf16),
 * s_j = w3 . relu(W2 relu(W1 x_j + b1) + b2) + b3 (bf16 MFMA operands, fp32
 * accumulation), the masked softmax / pooling of mrec_din_pool_fwd, and in the
 * backward the MLP recomputed, dX kept fp32 into the rows' gradient.
 *   rows    gathered bf16 rows [q (batch) | k (batch L)] (row stride ld_rows, 16-B
 *           aligned), his [batch, L] ids (validity: his > 0 or j == 0);
 *   w1 [H1, 4E] (ldw1), b1 [H1], w2 [H2, H1] (ldw2), b2 [H2], w3 [H2], b3 [1]:
 *           fp32 masters (nn.Linear layout; converted to bf16 in the kernel);
 *   fwd:    a [batch, L] softmax weights (saved for the backward), top [batch, ldt]
 *           = [q | u | 0-pad] bf16;
 *   bwd:    d_rows (same layout as rows) = the rows' bf16 gradient, part
 *           [parts][mrec_din_att_param_count] fp32 weight-gradient partials
 *           (parts = mrec_din_att_parts(batch));
 *   wgrad:  fixed-order sum of the partials into grads (flat [dW1 | dW2 | db1 | db2 |
 *           dw3 | db3]) or, with grads == NULL, SGD in place: p -= lr * grad.
 * Compiled shapes (mrec_din_att_supported): (E, H1, H2) with E in {16, 32} and
 * the tile counts of (32, 80, 40) (config C4) or (16, <= 32, <= 16); L <= 64.
 */
int32_t mrec_din_att_supported(int32_t E, int32_t H1, int32_t H2);
int64_t mrec_din_att_parts(int64_t batch);
int64_t mrec_din_att_param_count(int32_t E, int32_t H1, int32_t H2);
mrec_status mrec_din_att_fwd(const void *rows, int64_t ld_rows, const int32_t *his, int64_t ld_his,
                             int64_t batch, int32_t L, int32_t E, const float *w1, int64_t ldw1,
                             const float *b1, int32_t H1, const float *w2, int64_t ldw2,
                             const float *b2, int32_t H2, const float *w3, const float *b3,
                             float *a, void *top, int64_t ldt, mrec_stream stream);
mrec_status mrec_din_att_bwd(const void *rows, int64_t ld_rows, int64_t batch, int32_t L,
                             int32_t E, const float *w1, int64_t ldw1, const float *b1, int32_t H1,
                             const float *w2, int64_t ldw2, const float *b2, int32_t H2,
                             const float *w3, const float *b3, const float *a, const void *dtop,
                             int64_t lddt, void *d_rows, int64_t ld_drows, float *part,
                             int64_t parts, mrec_stream stream);
mrec_status mrec_din_att_wgrad(const float *part, int64_t parts, int32_t E, int32_t H1, int32_t H2,
                               float *grads, float lr, float *w1, int64_t ldw1, float *b1,
                               float *w2, int64_t ldw2, float *b2, float *w3, float *b3,
                               mrec_stream stream);

/*
 * Fused CTR head + BCE-with-logits (forward AND the loss gradient, one pass over h;
 * the train step of a Linear(H, 1) output layer on a ReLU MLP, the mean BCE loss):
 *   z[b]  = base[b] + bias + h[b] . w + xs[b, :ns] . ws + b2   (prediction logit;
 *           xs / ws / b2: an optional side linear term such as DeepFM's dense
 *           first-order weight and global bias, ns <= 64)
 *   dz[b] = (sigmoid(z[b]) - y[b]) / batch                       (d mean-loss / d z)
 *   dh[b, :] = dz[b] * w * (relu_mask ? h[b, :] > 0 : 1)          (bf16, pad columns 0)
 *   *loss = mean_b (max(z,0) - z y + log1p(exp(-|z|)))
 * and per-workgroup partials [dW (H) | sum dz | dws (ns)] in
 * part[mrec_ctr_head_parts(batch)][ldp >= H + 1 + ns].  The loss is reduced in the
 * same launch through loss_part[parts] and a ticket (*ticket must be 0 on entry and
 * is left 0).  H <= 1024, h / dh rows 16-byte aligned.
 * mrec_ctr_head_finish sums the partials in fixed order and, scaled by the
 * upstream gradient *g (NULL = 1), applies SGD (update: w -= lr g dW, ws -= lr g dws,
 * bias and b2 -= lr g sum dz) or writes dw_out / db_out / dws_out / db2_out.
 * Replaces Linear(H,1) + BCEWithLogitsLoss forward and backward (NCF.py:51,74 head;
 * losses.py:8-12 lacks BCE).
 */
int64_t mrec_ctr_head_parts(int64_t batch);
mrec_status mrec_ctr_head_fwd(const void *h, int64_t ldh, int64_t batch, int32_t H, const float *w,
                              const float *bias, const float *base, const float *y,
                              const float *xs, int64_t ldxs, int32_t ns, const float *ws,
                              const float *b2, int32_t relu_mask, float *z, float *dz, void *dh,
                              int64_t lddh, float *part, int64_t ldp, float *loss_part,
                              uint32_t *ticket, float *loss, mrec_stream stream);
mrec_status mrec_ctr_head_finish(const float *part, int64_t ldp, int64_t batch, int32_t H,
                                 int32_t ns, const float *g, int32_t update, float lr, float *w,
                                 float *bias, float *ws, float *b2, float *dw_out, float *db_out,
                                 float *dws_out, float *db2_out, mrec_stream stream);

/*
 * out[c] = sum_b s[b] X[b, c] for c < C, and *total = sum_b s[b] (if total != NULL):
 * the gradients of a small Linear / bias fed by per-sample scalars (dense
 * first-order weights, global bias, Linear(H, 1)).  One launch, one workgroup per
 * 8 columns, fixed-order tree reduction (deterministic).  With update != 0 the sums
 * are applied as SGD instead: out[c] -= lr * sum, *total -= lr * sum (fused
 * optimizer step of those parameters).
 */
mrec_status mrec_colsum(const float *s, const void *X, mrec_dtype x_dtype, int64_t ldx,
                        int64_t batch, int64_t C, float *out, float *total, int32_t update,
                        float lr, mrec_stream stream);

/* ------------------------------------------------------------------------- */
/* Ranking: pairwise losses, the positive's rank, negative sampling (ABI 31)  */
/* ------------------------------------------------------------------------- */
typedef enum {
  MREC_PAIR_BPR = 0, /* softplus(neg - pos), torch's softplus: x for x > 20, else log1p(exp(x))
                        (torchrec/loss/BPRLoss.py:15-23) */
  MREC_PAIR_TOP1 = 1 /* sigmoid(neg - pos) + sigmoid(neg^2)  (torchrec/loss/Top1Loss.py:14-22) */
} mrec_pair_kind;
typedef enum { MREC_REDUCE_NONE = 0, MREC_REDUCE_MEAN = 1, MREC_REDUCE_SUM = 2 } mrec_reduction;

/*
 * Pairwise ranking losses on x [batch, 2] fp32 (row stride ld >= 2 elements; column 0
 * the positive's score, column 1 the negative's), fp32 arithmetic.  `kind` is an
 * mrec_pair_kind and `reduction` an mrec_reduction (int32: an unknown value is
 * MREC_EINVAL).  Forward: out [batch] for NONE, else out [1] = the sum (SUM) or the sum
 * / batch (MEAN) by one workgroup in a fixed order (bitwise reproducible); batch 0
 * gives 0.  Backward: dx [batch, 2] (contiguous) = g * dl/dx, with the upstream
 * gradient g a DEVICE pointer: g[b] for NONE, g[0] for MEAN (also scaled by 1 / batch)
 * and SUM.  One kernel each way, no host sync.
 */
mrec_status mrec_pair_loss_fwd(const float *x, int64_t ld, int64_t batch, int32_t kind,
                               int32_t reduction, float *out, mrec_stream stream);
mrec_status mrec_pair_loss_bwd(const float *x, int64_t ld, int64_t batch, int32_t kind,
                               int32_t reduction, const float *g, float *dx, mrec_stream stream);

/*
 * Rank of column 0 in each row of pred [rows, n] fp32 (row stride ld >= n elements):
 *   rank[r] = 1 + #{j >= 1 : pred[r, j] > pred[r, 0]}        (int32 [rows])
 * so a tie resolves in the positive's favour (what a stable descending sort gives);
 * a NaN in column 0 gives rank n, a NaN in any other column never counts.  One wave
 * per row, several rows per workgroup, no atomics.  Replaces the argsort + argwhere of
 * IMetric.get_pos_rank (torchrec/metric/IMetric.py:17-26) on a leave-one-out
 * candidate list whose positive is first.
 */
mrec_status mrec_rank_pos(const float *pred, int64_t rows, int32_t n, int64_t ld, int32_t *rank,
                          mrec_stream stream);

/*
 * Negative sampling: out[b * n_neg + j] (int32 [batch, n_neg]) is an item of
 * [low, high) that user uids[b] (MREC_I32 / MREC_I64) has not interacted with.  The
 * users' items are a CSR: items[offsets[u] .. offsets[u + 1]) sorted ascending and
 * de-duplicated, offsets int64 [n_users + 1]; a uid outside [0, n_users) has no items.
 * With 64-bit wrapping arithmetic, G = 0x9E3779B97F4A7C15 and the splitmix64 finaliser
 *   mix(z): z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27;
 *           z *= 0x94D049BB133111EB; z ^= z >> 31
 * output i = b * n_neg + j has the key k = mix(mix(mix(seed + G) + step) + i), and its
 * attempt a = 0, 1, ... draws
 *   h = mix(k + (a + 1) * G),   item = low + (((h >> 32) * (high - low)) >> 32)
 * (multiply-shift of the hash's high half).  A draw found in the user's items (binary
 * search) is rejected and the next attempt drawn, MREC_NEG_MAX_ATTEMPTS at the most:
 * then the last draw is kept and *d_unresolved (device int32, required) is incremented
 * by one.  The result depends on (seed, step, batch, n_neg, ids) only, never on the
 * launch geometry.  Replaces rng.integers(low, high) + the `while neg in user set`
 * loop of SimpleDataReader.train_neg_sample (SimpleDataReader.py:280-300); numpy's
 * own stream is not reproduced.
 */
mrec_status mrec_neg_sample(const void *uids, mrec_dtype uid_dtype, int64_t batch, int32_t n_neg,
                            const int64_t *offsets, const int32_t *items, int64_t n_users,
                            int32_t low, int32_t high, uint64_t seed, uint64_t step, int32_t *out,
                            int32_t *d_unresolved, mrec_stream stream);

/* ------------------------------------------------------------------------- */
/* SASRec encoder, fused per sample (ABI 32; csrc/sasrec.hip)                  */
/* ------------------------------------------------------------------------- */
/*
 * The whole SASRec encoder (torchrec/model/SASRec.py:83-110) in one launch each way.
 * Per sample b, with valid_j = his[b, j] > 0 or j == 0:
 *   X      = bf16(rows[b L + j] + pos[(his_len[b] - j)]) at valid j, a zero row elsewhere
 *   num_layers x the ONE shared block:
 *     Q = X wq^T, K = X wk^T, A = softmax_k(D^-0.5 Q K^T) over valid keys (shifted by
 *     the row's own maximum), X <- bf16(LayerNorm(X + relu(A K w1^T + b1) w2^T + b2))
 *   v[b]   = sum_{valid j} X_j / his_len[b]                                  (fp32)
 * bf16 MFMA operands, fp32 accumulation / softmax / LayerNorm.  One description for
 * both directions; the forward ignores the backward's fields.
 *   rows    gathered item rows [batch L] bf16 (row stride ld_rows, a multiple of 8;
 *           16-B aligned); his [batch, L] (ld_his), his_len [batch]: int32;
 *   pos     position table [pos_rows, D] fp32 (ld_pos); a valid position whose id
 *           his_len - j falls outside [0, pos_rows) contributes no position row and
 *           sets *d_oob_flag = 1 (NULL: not reported), the bank's convention;
 *   wq, wk, w1, w2 [D, D] (ld_*), b1, b2, gamma, beta [D]: fp32 masters, nn.Linear
 *           layout, converted to bf16 in the kernel;
 *   hs      [num_layers, batch, L, D] bf16, contiguous: the layer outputs, written by
 *           the forward and read by the backward, which recomputes everything else;
 *   v       [batch, D] fp32 (forward);
 *   dv      [batch, D] fp32; d_rows (row stride ld_drows) the rows' bf16 gradient,
 *           bitwise zero at invalid positions; part [parts][mrec_sasrec_param_count]
 *           fp32 per-workgroup partials of every dense gradient, flat
 *           [dwq | dwk | dw1 | dw2 | db1 | db2 | dgamma | dbeta | dpos], summed over the
 *           workgroup's samples and the layers (parts = mrec_sasrec_parts(batch)).
 * mrec_sasrec_wgrad sums `count` columns of the partials in workgroup order into grads
 * (bit-reproducible).  Compiled shapes (mrec_sasrec_supported): D in {16, 32, 64},
 * 1 <= L <= 64.  Stream-ordered, no allocation; anything else is MREC_EINVAL.
 */
typedef struct {
  const void *rows;
  int64_t ld_rows;
  const int32_t *his;
  int64_t ld_his;
  const int32_t *his_len;
  const float *pos;
  int64_t ld_pos;
  int32_t pos_rows;
  const float *wq;
  int64_t ld_wq;
  const float *wk;
  int64_t ld_wk;
  const float *w1;
  int64_t ld_w1;
  const float *b1;
  const float *w2;
  int64_t ld_w2;
  const float *b2;
  const float *gamma;
  const float *beta;
  float eps;
  int32_t num_layers;
  int64_t batch;
  int32_t L;
  int32_t D;
  void *hs;
  float *v;
  int32_t *d_oob_flag;
  const float *dv;
  void *d_rows;
  int64_t ld_drows;
  float *part;
  int64_t parts;
} mrec_sasrec_args;

int32_t mrec_sasrec_supported(int32_t D, int32_t L);
int64_t mrec_sasrec_parts(int64_t batch);
int64_t mrec_sasrec_param_count(int32_t D, int32_t pos_rows);
mrec_status mrec_sasrec_fwd(const mrec_sasrec_args *args, mrec_stream stream);
mrec_status mrec_sasrec_bwd(const mrec_sasrec_args *args, mrec_stream stream);
mrec_status mrec_sasrec_wgrad(const float *part, int64_t parts, int64_t count, float *grads,
                              mrec_stream stream);

/* ------------------------------------------------------------------------- */
/* GRU4Rec session encoder, the whole recurrence per launch (ABI 33; csrc/gru.hip) */
/* ------------------------------------------------------------------------- */
/*
 * The GRU of torchrec/model/GRU4Rec.py:51-56 (nn.GRU over the packed history, one
 * layer, h_-1 = 0) in one launch each way.  Per sample b, for t = 0 .. his_len[b] - 1:
 *   x_t = rows[b L + t]
 *   r_t = sigmoid(W_ir x_t + b_ir + W_hr h_{t-1} + b_hr)
 *   z_t = sigmoid(W_iz x_t + b_iz + W_hz h_{t-1} + b_hz)
 *   n_t = tanh(W_in x_t + b_in + r_t (W_hn h_{t-1} + b_hn))
 *   h_t = (1 - z_t) n_t + z_t h_{t-1};      h_last[b] = h_{his_len[b] - 1}
 * x, the two weight matrices and h as a product's operand are rounded to bf16, every
 * product accumulates in fp32, the gate math and the carried h are fp32.  A position is
 * live iff t < his_len[b]; rows at other positions are never read.
 *   rows    bf16 gathered rows [batch * L], row stride ld_rows elements (16-byte aligned
 *           rows: ld_rows a multiple of 8);
 *   his_len int32 [batch]; a length outside 1 .. L sets *d_oob_flag (may be NULL) and is
 *           clamped into 0 .. L (0: h_last = 0), nothing is read out of bounds;
 *   order   int32 [batch] or NULL: tile slot -> sample, a permutation that puts samples of
 *           similar length into the same 16-sample tile (speed only: a sample's bits do
 *           not depend on it); an entry outside the batch sets the flag and is skipped;
 *   w_ih [3H, E], w_hh [3H, H] (row strides ld_ih, ld_hh), b_ih, b_hh [3H]: the fp32
 *           masters in nn.GRU's layout, gate order r, z, n;
 *   hs      [batch, L, H] fp32, the hidden sequence as the forward carried it, written at
 *           live positions (forward) and read by the backward, which recomputes the gates;
 *   h_last  [batch, H] fp32 (forward);
 *   dh_last [batch, H] fp32; d_rows (row stride ld_drows) the rows' bf16 gradient,
 *           bitwise zero at t >= his_len; part [parts][mrec_gru_param_count] fp32
 *           per-workgroup partials of the dense gradients, flat
 *           [dW_ih | dW_hh | db_ih | db_hh] (parts = mrec_gru_parts(batch)), to be summed
 *           in workgroup order by mrec_sasrec_wgrad (bit-reproducible).
 * Compiled shapes (mrec_gru_supported): E, H in {16, 32, 64}, 1 <= L <= 64.  A workgroup
 * takes mrec_gru_tile() samples at a time.  Stream-ordered, no allocation; anything
 * else is MREC_EINVAL before any device work.
 */
typedef struct {
  const void *rows;
  int64_t ld_rows;
  const int32_t *his_len;
  const int32_t *order;
  const float *w_ih;
  int64_t ld_ih;
  const float *w_hh;
  int64_t ld_hh;
  const float *b_ih;
  const float *b_hh;
  int32_t E;
  int32_t H;
  int32_t L;
  int64_t batch;
  void *hs;
  float *h_last;
  int32_t *d_oob_flag;
  const float *dh_last;
  void *d_rows;
  int64_t ld_drows;
  float *part;
  int64_t parts;
} mrec_gru_args;

int32_t mrec_gru_supported(int32_t E, int32_t H, int32_t L);
int32_t mrec_gru_tile(void);
int64_t mrec_gru_parts(int64_t batch);
int64_t mrec_gru_param_count(int32_t E, int32_t H);
mrec_status mrec_gru_fwd(const mrec_gru_args *args, mrec_stream stream);
mrec_status mrec_gru_bwd(const mrec_gru_args *args, mrec_stream stream);

/* ------------------------------------------------------------------------- */
/* NCF / NeuMF pair scorer, the whole scorer per launch (ABI 34; csrc/ncf.hip)  */
/* ------------------------------------------------------------------------- */
/*
 * The scorer of torchrec/model/NCF.py:62-74 in one launch each way.  Per pair p:
 *   rows[p] = [mf_u | mf_i | mlp_u | mlp_i]   (4 E bf16, what one gather over the bank
 *                                              [users, items, users, items] returns)
 *   g       = mf_u * mf_i                                                   [E]
 *   h_0     = [mlp_u | mlp_i],  h_{l+1} = relu(w[l] h_l + b[l])   l = 0 .. n_layers - 1
 *   pred[p] = wp . [g | h_k]
 * Each weight matrix is rounded to bf16 once, an activation is rounded to bf16 exactly
 * where it becomes the next layer's operand; every product accumulates in fp32, bias and
 * ReLU are fp32, g and the final dot are fp32 from the bf16 rows and the fp32 wp (h_k is
 * not rounded).  One description for both directions; the forward ignores the
 * backward's fields and saves nothing: the backward recomputes it with the same MFMAs.
 *   rows    bf16 [pairs] rows, row stride ld_rows elements (16-byte aligned rows:
 *           ld_rows a multiple of 8, >= 4 E);
 *   widths  the n_layers hidden widths; w[l] [widths[l], widths[l-1]] (widths[-1] = 2 E,
 *           row stride ld_w[l]), b[l] [widths[l]], wp [E + widths[n_layers-1]]: the fp32
 *           masters in nn.Linear layout;
 *   pred    [pairs] fp32 (forward);
 *   dpred   [pairs] fp32; d_rows (row stride ld_drows, a multiple of 8, >= 4 E) the rows'
 *           bf16 gradient in the rows' layout, one rounding from fp32; columns >= 4 E and
 *           rows >= pairs are not written; part [parts][mrec_ncf_param_count] fp32
 *           per-workgroup partials of the dense gradients, flat
 *           [dw[0] | .. | dw[k-1] | db[0] | .. | db[k-1] | dwp], each dw[l] dense
 *           [widths[l], widths[l-1]] (parts = mrec_ncf_parts(pairs)), to be summed in
 *           workgroup order by mrec_sasrec_wgrad.  No atomics: two runs give equal bits,
 *           and a pair's bits do not depend on its place in the batch.
 * Compiled shapes (mrec_ncf_supported, decided from the shape alone): E in {8, 16, 32,
 * 64}, 1 .. 3 layers, widths multiples of 8 in 8 .. 128, as long as the bf16 weight
 * images and the tile buffers fit a CU's 160 KB of LDS and the weight gradients fit the
 * accumulator registers (at most 128 tiles of 16 x 16): every tower that narrows from
 * 128, such as (64, [128, 64, 32]), and (64, [128, 128]) fit; (64, [128, 128, 128]) does
 * not.  A workgroup takes mrec_ncf_tile() pairs at a time.  Stream-ordered, no
 * allocation, no pointer kept; anything else is MREC_EINVAL before any device work.
 */
typedef struct {
  const void *rows;
  int64_t ld_rows;
  int64_t pairs;
  int32_t E;
  int32_t n_layers;
  int32_t widths[3];
  const float *w[3];
  int64_t ld_w[3];
  const float *b[3];
  const float *wp;
  float *pred;
  const float *dpred;
  void *d_rows;
  int64_t ld_drows;
  float *part;
  int64_t parts;
} mrec_ncf_args;

int32_t mrec_ncf_supported(int32_t E, int32_t n_layers, const int32_t *widths);
int32_t mrec_ncf_tile(void);
int64_t mrec_ncf_parts(int64_t pairs);
int64_t mrec_ncf_param_count(int32_t E, int32_t n_layers, const int32_t *widths);
mrec_status mrec_ncf_fwd(const mrec_ncf_args *args, mrec_stream stream);
mrec_status mrec_ncf_bwd(const mrec_ncf_args *args, mrec_stream stream);

/* ------------------------------------------------------------------------- */
/* Retrieval: full-catalogue top-K, score and select fused (ABI 35; csrc/topk.hip) */
/* ------------------------------------------------------------------------- */
/*
 * For queries q [batch, D] (MREC_F32 or MREC_BF16, row stride ldq elements) and table
 * `table` of `bank` (D = bank->dim), restricted to the table-local item ids [low, high):
 *   score[b, i] = sum_d bf16(q[b, d]) * bf16(T[i, d])      fp32 accumulation
 *                 + w[i]                                    fp32, only with use_w (has_w bank)
 * bf16() is round-to-nearest-even: exact for a bf16 bank, and for an fp32 bank the rounding
 * a gather of its rows as bf16 applies.  out_ids [batch, k] (int32, table-local) and
 * out_scores [batch, k] (fp32), common row stride ld_out >= k elements, receive per query
 * the k best eligible items sorted by the total order SCORE DESCENDING, THEN ID ASCENDING.
 * Columns >= k and rows >= batch of the outputs are not written.
 *   Eligibility.  Item i is eligible iff low <= i < high, its score is not NaN and it is
 *     not excluded.  +0.0 and -0.0 compare equal (the lower id wins; a zero is returned
 *     as +0.0).  With fewer than k eligible items the remaining slots hold id -1 and score
 *     -inf; an item whose score is -inf is returned as such a slot.
 *   Exclusion (optional; all NULL / 0 for none).  A CSR: excl_items[excl_offsets[r] ..
 *     excl_offsets[r + 1]) (int32, table-local ids, sorted ascending and de-duplicated;
 *     excl_offsets int64 [excl_n_rows + 1]) are the items excluded for CSR row r -- the
 *     layout mrec_neg_sample reads.  Query b uses row excl_row[b] (excl_row_dtype MREC_I32
 *     or MREC_I64), or row b when excl_row is NULL; a row index outside [0, excl_n_rows)
 *     excludes nothing.  An item is looked up (binary search) only when it would otherwise
 *     enter the query's kept list, never for every score.
 *   Determinism.  The total order makes the answer unique, and the result depends on the
 *     inputs only: never on the launch geometry, on `splits`, on where the bank lies or on
 *     the order in which candidates arrive.  Two runs, or two split counts, give equal bits.
 *   Never read: the pad columns of a bank row past [v | w] (w itself only with use_w),
 *     rows outside [row_offset[table] + low, row_offset[table] + high), columns >= D of q.
 *     The rows are read as stored: a bank under the lazy fused Adam is flushed first
 *     (mrec_emb_optim_flush).
 *   splits: the item range is cut into `splits` parts scanned by different workgroups, 0 =
 *     mrec_topk_splits(batch, high - low), at most 64.  With more than one split the
 *     partial lists go through `workspace` (8-byte aligned,
 *     mrec_topk_workspace_size(batch, k, splits) bytes; splits = 0 there sizes for any
 *     default) and a second launch merges them.
 * Compiled shapes (mrec_topk_supported): D in {8, 16, 32, 64}, 1 <= k <= 128, bank F32 or
 * BF16; batch >= 0 and high - low >= 0 (an empty batch writes nothing, an empty range fills
 * the padding values).  A workgroup carries mrec_topk_tile_queries() queries and streams
 * mrec_topk_tile_items() items at a time.  Caller-owned buffers, no allocation, no host
 * synchronisation, all work on `stream`; anything else is MREC_EINVAL with
 * mrec_last_error() before any launch.
 */
typedef struct {
  const mrec_table_bank *bank;
  int32_t table;
  int64_t low;
  int64_t high;
  const void *q;
  mrec_dtype q_dtype;
  int64_t ldq;
  int64_t batch;
  int32_t k;
  int32_t use_w;
  const int64_t *excl_offsets;
  const int32_t *excl_items;
  int64_t excl_n_rows;
  const void *excl_row;
  mrec_dtype excl_row_dtype;
  int32_t splits;
  void *workspace;
  size_t workspace_bytes;
  int32_t *out_ids;
  float *out_scores;
  int64_t ld_out;
} mrec_topk_args;

int32_t mrec_topk_supported(int32_t D, int32_t k, mrec_dtype bank_dtype);
int32_t mrec_topk_tile_queries(void); /* queries a workgroup carries */
int32_t mrec_topk_tile_items(void);   /* items per streamed tile     */
int32_t mrec_topk_splits(int64_t batch, int64_t n_items); /* the default item-split count */
size_t mrec_topk_workspace_size(int64_t batch, int32_t k, int32_t splits);
mrec_status mrec_topk(const mrec_topk_args *args, mrec_stream stream);

/* ------------------------------------------------------------------------- */
/* NCF retrieval: full-catalogue top-K with the NeuMF scorer (ABI 36; csrc/ncf_topk.hip) */
/* ------------------------------------------------------------------------- */
/*
 * For the users uid [batch] (MREC_I32 or MREC_I64) and every item i of the table-local
 * range [low, high), the score of mrec_ncf_fwd for the pair (u = uid[b], i) -- without the
 * gathered row and without the [batch, items] scores ever reaching memory -- fused with
 * the selection of mrec_topk.  The four tables are tables of one bank (E = bank->dim):
 * table_mf_u and table_mlp_u have one row per user, table_mf_i and table_mlp_i one per
 * item.  The score contract: every table element is used as its bf16 value (round to
 * nearest even from an fp32 bank: what a gather of the row as bf16 gives), every w[l] is
 * rounded to bf16 once per workgroup, and
 *   a[b, n]   = b[0][n] + sum_e w[0][n, e]     * mlp_u[u, e]      fp32, once per user
 *   c[i, n]   =           sum_e w[0][n, E + e] * mlp_i[i, e]      fp32, once per item (tile)
 *   h_1       = relu(a[b] + c[i])
 *   h_{l+1}   = relu(w[l] h_l + b[l])     l = 1 .. n_layers - 1, as mrec_ncf_fwd computes it
 *   score     = sum_e wp[e] * (mf_u[u, e] * mf_i[i, e])  +  wp[E:] . h_{n_layers}
 * relu(x) is mrec_ncf_fwd's `x > 0 ? x : 0`: a NaN pre-activation gives 0, so a NaN in an mlp
 * row does not reach the score; a NaN in an mf row does, and that item is not eligible.
 * The rounding points are mrec_ncf_fwd's: each h_l is rounded to bf16 where it becomes the
 * next layer's operand; the last layer's output, g = mf_u * mf_i and the final dot stay
 * fp32 (with one layer h_1 is the last and is not rounded).  Against mrec_ncf_fwd only the
 * fp32 summation order of layer 0 differs (its user half and its item half are summed
 * separately).  A pair's score bits depend on the pair alone: not on its tile, its place
 * in the batch, the split count or where the bank lies.
 *   Selection.  Eligibility, exclusion (excl_* as in mrec_topk_args, row b of the CSR or
 *     row excl_row[b]), the total order SCORE DESCENDING, THEN ID ASCENDING, the padding
 *     (id -1, score -inf), `splits` and the workspace are those of mrec_topk, word for
 *     word; a NaN score is never returned; two runs, or two split counts, give equal bits.
 *   User ids.  A uid outside [0, rows of the user tables) is never used as a table index:
 *     it sets *d_oob_flag to 1 (when non-NULL) and its output row is all padding.
 *   Never read: the pad columns of a bank row past the embedding, item rows outside
 *     [low, high), user rows no uid names.  The rows are read as stored: a bank under the
 *     lazy fused Adam is flushed first (mrec_emb_optim_flush).
 * widths, w, ld_w, b, wp: the fp32 masters in nn.Linear layout, as in mrec_ncf_args (w[0]
 * is [widths[0], 2 E]).  Compiled shapes (mrec_ncf_topk_supported, decided from the shape
 * alone): those of mrec_ncf_supported -- E in {8, 16, 32, 64}, 1 .. 3 layers, widths
 * multiples of 8 in 8 .. 128 -- with 1 <= k <= 128 and an F32 or BF16 bank, as long as the
 * weight images, the tile buffers and the per-user key buffers (which grow with k) fit a
 * CU's 160 KB of LDS: (64, [128, 64, 32]) fits at k = 128.  A workgroup carries
 * mrec_ncf_topk_tile_users() users and streams mrec_ncf_topk_tile_items() items at a time;
 * mrec_ncf_topk_splits(batch, high - low) is the default split count, and
 * mrec_ncf_topk_workspace_size(batch, k, splits) sizes the workspace (8-byte aligned;
 * splits = 0 sizes for any default).  batch >= 0 and high - low >= 0 (an empty batch writes
 * nothing, an empty range fills the padding values).  Caller-owned buffers, no allocation,
 * no host synchronisation, all work on `stream`; anything else is MREC_EINVAL with
 * mrec_last_error() before any launch.
 */
typedef struct {
  const mrec_table_bank *bank;
  int32_t table_mf_u;
  int32_t table_mf_i;
  int32_t table_mlp_u;
  int32_t table_mlp_i;
  int64_t low;
  int64_t high;
  const void *uid;
  mrec_dtype uid_dtype;
  int64_t batch;
  int32_t n_layers;
  int32_t widths[3];
  const float *w[3];
  int64_t ld_w[3];
  const float *b[3];
  const float *wp;
  int32_t k;
  int32_t splits;
  const int64_t *excl_offsets;
  const int32_t *excl_items;
  int64_t excl_n_rows;
  const void *excl_row;
  mrec_dtype excl_row_dtype;
  int32_t *d_oob_flag;
  void *workspace;
  size_t workspace_bytes;
  int32_t *out_ids;
  float *out_scores;
  int64_t ld_out;
} mrec_ncf_topk_args;

int32_t mrec_ncf_topk_supported(int32_t E, int32_t n_layers, const int32_t *widths, int32_t k,
                                mrec_dtype bank_dtype);
int32_t mrec_ncf_topk_tile_users(void); /* users a workgroup carries */
int32_t mrec_ncf_topk_tile_items(void); /* items per streamed tile   */
int32_t mrec_ncf_topk_splits(int64_t batch, int64_t n_items); /* the default item-split count */
size_t mrec_ncf_topk_workspace_size(int64_t batch, int32_t k, int32_t splits);
mrec_status mrec_ncf_topk(const mrec_ncf_topk_args *args, mrec_stream stream);

/* ------------------------------------------------------------------------- */
/* Shared negatives: list-wise losses over one pool of negatives shared by the */
/* batch, loss and gradients fused with the scores (ABI 37; csrc/shneg.hip)    */
/* ------------------------------------------------------------------------- */
/*
 * Inputs.  q [batch, D] (q_dtype MREC_F32 or MREC_BF16, row stride ldq elements), the
 * gathered item rows pos [batch, D] and neg [n_neg, D] of ONE dtype (row_dtype MREC_F32 or
 * MREC_BF16; row strides ld_pos, ld_neg); neg may alias pos (in-batch negatives).  Optional
 * pos_id [batch] and neg_id [n_neg] (id_dtype MREC_I32 or MREC_I64, both NULL or both
 * given): candidate j is MASKED for query b iff neg_id[j] == pos_id[b]; without ids nothing
 * is masked.  Optional pos_bias [batch], neg_bias [n_neg]: fp32 constants added to the
 * scores (the log-Q correction); they get no gradient.
 *   s[b, j] = sum_d bf16(q[b, d]) * bf16(neg[j, d]) (+ neg_bias[j])
 *   s+[b]   = sum_d bf16(q[b, d]) * bf16(pos[b, d]) (+ pos_bias[b])
 * bf16() is round-to-nearest-even (mrec_topk's operand rounding: exact for bf16 operands),
 * every product accumulates in fp32 (s through the MFMA, s+ as an fmaf chain).  E_b is the
 * set of unmasked candidates of query b, n_b = |E_b|.  Per-query loss (kind):
 *   MREC_SHNEG_SOFTMAX  L_b = log(exp(s+[b]) + sum_{j in E_b} exp(s[b, j])) - s+[b]
 *                       an online log-sum-exp with a running maximum: safe for scores of
 *                       any magnitude
 *   MREC_SHNEG_BPR      L_b = (1 / n_b) sum_{j in E_b} softplus(s[b, j] - s+[b])
 *                       (mrec_pair_loss_fwd's MREC_PAIR_BPR of each pair, averaged)
 *   MREC_SHNEG_TOP1     L_b = (1 / n_b) sum_{j in E_b} sigmoid(s[b, j] - s+[b]) + sigmoid(s[b, j]^2)
 *                       (MREC_PAIR_TOP1 in the same way)
 * n_b = 0 (n_neg = 0 included) gives L_b = 0 and zero gradients for every kind; batch = 0
 * launches nothing and writes nothing.  reduction: MREC_REDUCE_NONE writes loss [batch];
 * MEAN / SUM write loss [1], a fixed-order reduction of the L_b (one workgroup, as
 * mrec_pair_loss_fwd), the L_b themselves going through the workspace.
 *   The forward also writes stats [batch][4] fp32 -- s+[b], the maximum M_b over s+[b] and
 * the unmasked s[b, j], the sum exp(s+ - M_b) + sum_j exp(s[b, j] - M_b) (softmax only), n_b
 * -- which is all the backward keeps: it recomputes every score tile with the same MFMAs.
 * Gradients, with g the upstream gradient on the device ([batch] for NONE, [1] otherwise;
 * g_b = g[b], g[0] / batch or g[0]) and c_b = g_b / sum_b (softmax) or g_b / n_b (bpr, top1):
 *   a[b, j] = g_b dL_b/ds[b, j]   softmax exp(s[b, j] - M_b) c_b;  bpr softplus'(x) c_b;
 *                                 top1 (sigmoid'(x) + 2 s[b, j] sigmoid'(s[b, j]^2)) c_b;
 *                                 x = s[b, j] - s+[b];  0 where masked
 *   a[b, +] = g_b dL_b/ds+[b]     softmax exp(s+[b] - M_b) c_b - g_b;  bpr, top1 minus the
 *                                 fp32 sum over j of the first term of a[b, j]
 *   dq[b]   = sum_j a[b, j] bf16(neg[j]) + a[b, +] bf16(pos[b])       in q's dtype
 *   dpos[b] = a[b, +] bf16(q[b])                                      in the rows' dtype
 *   dneg[j] = sum_b a[b, j] bf16(q[b])                                in the rows' dtype
 * Rounding points: each a[b, j] enters the MFMAs of the two sums over j and over b as
 * hi + lo, two bf16 values (hi = bf16(a), lo = bf16(a - hi): 2^-16 relative each; a
 * coefficient that is a bf16 value is exact); a[b, +] and the products with it stay fp32; every sum accumulates in fp32 and each output is rounded once.  A candidate that is
 * masked for every query contributes exactly nothing, whatever its row holds (its row is
 * replaced by zeros where no coefficient of a 32 x 32 tile uses it), and its dneg is 0; a
 * non-finite row that some query does use may reach the gradients of its tile's queries.
 *   Determinism.  The outputs are a function of the inputs alone: no floating-point
 * atomics, every sum in a fixed order (per 1024 streamed rows one MFMA chain per wave, the
 * four waves in order, then the chunks of 1024 in order).  `splits` cuts the batch of the
 * candidate-major pass (dneg) into parts run by different workgroups, 0 =
 * mrec_shneg_splits(batch, n_neg), at most 64: it moves whole chunks only, their partials
 * go through `workspace` and are summed in the same order, so the bits do not depend on
 * it, on the grid, on where the operands lie or on the run.
 *   workspace: 16-byte aligned, mrec_shneg_workspace_size(batch, n_neg, D, splits) bytes
 * (splits = 0 there sizes for any default); used by the forward for MEAN / SUM and by the
 * backward when more than one split runs.  One description for both directions: the forward
 * ignores g and the gradients' fields, the backward ignores loss.
 * Compiled shapes (mrec_shneg_supported): D in {8, 16, 32, 64}, q and rows F32 or BF16, any
 * batch and n_neg up to 2^31 - 1.  q, pos and neg need 16-byte aligned rows (pointer and
 * row stride in bytes multiples of 16); the outputs any row stride >= D.  A workgroup holds
 * mrec_shneg_tile_queries() queries (forward, query-major pass) or
 * mrec_shneg_tile_candidates() candidates (candidate-major pass).  Never read: columns >= D
 * of any row; never written: columns >= D and rows past the shape.  Caller-owned buffers,
 * no allocation, no host synchronisation, all work on `stream`; anything else is
 * MREC_EINVAL with mrec_last_error() before any launch.
 * mrec_shneg_math_probe applies one of the device functions the losses call to x [n] fp32
 * -- fn 0 expf, 1 logf, 2 softplus, 3 sigmoid, 4 sigmoid' -- so that their error can be
 * measured alone (the tests' tolerance).
 */
typedef enum { MREC_SHNEG_SOFTMAX = 0, MREC_SHNEG_BPR = 1, MREC_SHNEG_TOP1 = 2 } mrec_shneg_kind;

typedef struct {
  const void *q;
  mrec_dtype q_dtype;
  int64_t ldq;
  const void *pos;
  int64_t ld_pos;
  const void *neg;
  int64_t ld_neg;
  mrec_dtype row_dtype;
  int64_t batch;
  int64_t n_neg;
  int32_t D;
  const void *pos_id;
  const void *neg_id;
  mrec_dtype id_dtype;
  const float *pos_bias;
  const float *neg_bias;
  int32_t kind;
  int32_t reduction;
  float *loss;
  float *stats;
  const float *g;
  void *dq;
  int64_t ld_dq;
  void *dpos;
  int64_t ld_dpos;
  void *dneg;
  int64_t ld_dneg;
  int32_t splits;
  void *workspace;
  size_t workspace_bytes;
} mrec_shneg_args;

int32_t mrec_shneg_supported(int32_t D, mrec_dtype q_dtype, mrec_dtype row_dtype);
int32_t mrec_shneg_tile_queries(void);    /* queries a workgroup holds    */
int32_t mrec_shneg_tile_candidates(void); /* candidates a workgroup holds */
int32_t mrec_shneg_splits(int64_t batch, int64_t n_neg); /* the default batch-split count */
size_t mrec_shneg_workspace_size(int64_t batch, int64_t n_neg, int32_t D, int32_t splits);
mrec_status mrec_shneg_loss_fwd(const mrec_shneg_args *args, mrec_stream stream);
mrec_status mrec_shneg_loss_bwd(const mrec_shneg_args *args, mrec_stream stream);
mrec_status mrec_shneg_math_probe(int32_t fn, const float *x, int64_t n, float *y, mrec_stream stream);

/* ------------------------------------------------------------------------- */
/* DLRM dot interaction: all pairwise dot products of a sample's embedding     */
/* rows and its bottom-MLP vector, one launch each way (ABI 38;                */
/* csrc/dot_interact.hip)                                                      */
/* ------------------------------------------------------------------------- */
/*
 * Per sample b, with n = n_fields + 1 vectors of D elements:
 *   t_0 = bot[b]                       the bottom-MLP output, [batch, D], row stride ld_bot
 *   t_i = rows[b, (i-1) D : i D]       the gathered rows, [batch, n_fields * D], the layout
 *                                      mrec_emb_gather_fwd writes, row stride ld_rows
 *   z[i, j]                = sum_d bf16(t_i[d]) * bf16(t_j[d])     0 <= j < i < n
 *   x[b, 0 : D]            = t_0                                   (in x's dtype)
 *   x[b, D + i(i-1)/2 + j] = z[i, j]          P = n (n - 1) / 2 pairs, the order of the
 *                                             strict lower triangle read row by row
 *   x[b, D + P : x_cols]   = 0                x_cols >= D + P given by the caller
 * bf16() is round-to-nearest-even (mrec_topk's operand rounding: exact for bf16 operands);
 * the products accumulate in fp32 through the MFMA and each z is rounded once, into x's
 * dtype.  bot may be NULL: there is no bottom vector, n = n_fields, t_i = rows[b, i D :
 * (i+1) D], x starts with the pairs (x_cols >= P) and dbot is ignored.
 *   Backward, from dx [batch, >= D + P] (row stride ld_dx), bot and rows again -- nothing
 * else is kept from the forward:
 *   G symmetric n x n:  G[i, j] = G[j, i] = dx[b, D + i(i-1)/2 + j]  (i > j),  G[i, i] = 0
 *   dt_i[d]  = sum_j G[i, j] * bf16(t_j[d])                         fp32 accumulation
 *   dbot[b]  = dt_0 + dx[b, 0 : D]                                  in bot's dtype
 *   drows[b, (i-1) D : i D] = dt_i                                  in the rows' dtype
 * A bf16 dx enters the MFMA exactly; an fp32 dx enters as hi + lo, two bf16 values (hi =
 * bf16(g), lo = bf16(g - hi), as mrec_shneg_loss_bwd's coefficients: 2^-16 relative).  Each
 * output is rounded once.
 *   Determinism.  A sample's outputs are a function of that sample's inputs alone: one wave
 * per sample, no atomics, no sum across waves, so the bits do not depend on the batch, the
 * grid, the sample's position or the run.
 *   One description for both directions: the forward ignores dx, dbot and drows; the
 * backward ignores x and x_cols.
 * Compiled shapes (mrec_dot_interact_supported): D in {8, 16, 32, 64, 128}, 1 <= n_fields
 * <= 31, bot, rows, x and dx each MREC_F32 or MREC_BF16, independently; any batch up to
 * 2^31 - 1 (batch = 0 launches nothing).  Every operand and output needs 16-byte aligned
 * rows (pointer and row stride in bytes multiples of 16) of at least its width.  Never read:
 * columns >= D of a bot row, >= n_fields * D of a rows row, >= D + P of a dx row; never
 * written: columns >= x_cols of x, >= D of dbot, >= n_fields * D of drows, and rows >= batch.
 * Caller-owned buffers, no allocation, no host synchronisation, all work on `stream`;
 * anything else is MREC_EINVAL with mrec_last_error() before any launch.
 */
typedef struct {
  const void *bot;
  mrec_dtype bot_dtype;
  int64_t ld_bot;
  const void *rows;
  mrec_dtype rows_dtype;
  int64_t ld_rows;
  int64_t batch;
  int32_t n_fields;
  int32_t D;
  void *x;
  mrec_dtype x_dtype;
  int64_t ld_x;
  int64_t x_cols;
  const void *dx;
  mrec_dtype dx_dtype;
  int64_t ld_dx;
  void *dbot;
  int64_t ld_dbot;
  void *drows;
  int64_t ld_drows;
} mrec_dot_interact_args;

int32_t mrec_dot_interact_supported(int32_t D, int32_t n_fields, mrec_dtype bot_dtype,
                                    mrec_dtype rows_dtype, mrec_dtype x_dtype, mrec_dtype dx_dtype);
mrec_status mrec_dot_interact_fwd(const mrec_dot_interact_args *args, mrec_stream stream);
mrec_status mrec_dot_interact_bwd(const mrec_dot_interact_args *args, mrec_stream stream);

/* ------------------------------------------------------------------------- */
/* CIN: xDeepFM's Compressed Interaction Network, one layer per call (ABI 39;  */
/* csrc/cin.hip)                                                               */
/* ------------------------------------------------------------------------- */
/*
 * With m = n_fields, X^0 = x0 read as [batch, m, D] (d fastest, row stride ld_x0) and
 * X^{k-1} = xp read as [batch, H_prev, D] (row stride ld_xp; layer 1: xp = x0, H_prev = m):
 *   X^k[b, h, d] = sum_{i < H_prev} sum_{j < m} W[h, i, j] * X^{k-1}[b, i, d] * X^0[b, j, d]
 *   p[b, h]      = sum_d X^k[b, h, d]                       fp32, row stride ld_p
 * Identity activation, no bias, every map feeds both p and the next layer.
 *   Rounding.  x0, xp, W and dX^k enter the products as bf16 (RNE where stored in fp32; W
 * through its images).  Z = bf16(xp * x0) is rounded once.  Accumulation is fp32 (MFMA).  p
 * is summed from the fp32 accumulators; xk is rounded once when x_dtype is MREC_BF16.
 *   Weight images (bf16, built by the caller whenever W changes; pad entries are zero):
 *   w_fwd [mrec_cin_fwd_rows(H)][H_prev * MP]     w_fwd[h][i * MP + j] = W[h, i, j]
 *   w_bwd [r32(H_prev * MP)][mrec_cin_bwd_cols(H)] w_bwd[i * MP + j][h] = W[h, i, j]
 * MP = mrec_cin_field_pitch(n_fields) (16 or 32), r32 rounds up to a multiple of 32.
 *   Backward (mrec_cin_bwd: one data-gradient launch and one weight-gradient launch).
 * dX^k is dxk [batch, H, D] in x_dtype when given, else dp[b, h] broadcast over d (the last
 * layer).  With g = bf16(dX^k):
 *   dZ[b, (i, j), d]   = sum_h g[b, h, d] W[h, i, j]                    fp32, never stored
 *   dxp[b, i, d]       = sum_j dZ X^0[b, j, d]  (+ dp_prev[b, i] when dp_prev is given)
 *   dx0[b, j * D + d] += sum_i dZ X^{k-1}[b, i, d]                      fp32 accumulator
 *   dw[h, i, j]        = sum_{b, d} g[b, h, d] * bf16(xp[b, i, d] * x0[b, j, d])
 * dxp is rounded once into dxp_dtype.  dx0 is read and written by exactly one lane per
 * element; the caller zeroes it before the first (topmost) layer's call.  For layer 1 xp is
 * x0 and the caller adds dxp into dx0.  dw [H, H_prev, m] is contiguous fp32, overwritten.
 *   Determinism: no atomics; xk, p, dxp and dx0 of a sample depend on that sample alone;
 * dw is reduced over the batch in one fixed order by the one workgroup that owns the tile.
 *   One description for both directions: the forward ignores the backward fields and w_bwd,
 * the backward ignores xk, p and w_fwd.
 * Compiled shapes (mrec_cin_supported): 2 <= n_fields <= 32, D in {8, 16, 32, 64}, H a
 * multiple of 8 up to 256, H_prev the same or equal to n_fields; every dtype MREC_F32 or
 * MREC_BF16.  x0, xp, xk, dxk, dxp and the images need 16-byte aligned rows.  batch = 0
 * launches nothing.  Never read or written: columns past the stated widths, rows >= batch.
 * Anything else is MREC_EINVAL with mrec_last_error() before any launch.
 */
typedef struct {
  const void *x0;
  mrec_dtype x0_dtype;
  int64_t ld_x0;
  const void *xp;
  mrec_dtype xp_dtype;
  int64_t ld_xp;
  const void *w_fwd;
  int64_t ld_w_fwd;
  const void *w_bwd;
  int64_t ld_w_bwd;
  int64_t batch;
  int32_t n_fields;
  int32_t D;
  int32_t H_prev;
  int32_t H;
  mrec_dtype x_dtype; /* of xk and dxk */
  void *xk;
  int64_t ld_xk;
  float *p;
  int64_t ld_p;
  const void *dxk;
  int64_t ld_dxk;
  const float *dp;
  int64_t ld_dp;
  const float *dp_prev;
  int64_t ld_dp_prev;
  void *dxp;
  mrec_dtype dxp_dtype;
  int64_t ld_dxp;
  float *dx0;
  int64_t ld_dx0;
  float *dw;
} mrec_cin_args;

int32_t mrec_cin_supported(int32_t n_fields, int32_t D, int32_t H_prev, int32_t H,
                           mrec_dtype x0_dtype, mrec_dtype x_dtype);
int32_t mrec_cin_field_pitch(int32_t n_fields); /* MP */
int32_t mrec_cin_fwd_rows(int32_t H);           /* rows of w_fwd */
int32_t mrec_cin_bwd_cols(int32_t H);           /* columns of w_bwd */
mrec_status mrec_cin_fwd(const mrec_cin_args *args, mrec_stream stream);
mrec_status mrec_cin_bwd(const mrec_cin_args *args, mrec_stream stream);

/* ------------------------------------------------------------------------- */
/* AutoInt: one interacting layer (multi-head self-attention over the fields)  */
/* per call (ABI 40; csrc/autoint.hip)                                         */
/* ------------------------------------------------------------------------- */
/*
 * With m = n_fields, X = x read as [batch, m, d_in] (row stride ld_x), A = heads * head_dim
 * and the weights Wq, Wk, Wv, Wres in nn.Linear layout [A, d_in] (Wres optional: has_res):
 *   Q = X Wq^T, K = X Wk^T, V = X Wv^T                 [m, A], heads of head_dim columns
 *   S_h = scale * Q_h K_h^T                            [m, m] per head
 *   P_h = softmax over the keys (last index), shifted by the row's own maximum
 *   O   = [P_1 V_1 | .. | P_heads V_heads]             [m, A]
 *   Y   = relu(O + X Wres^T)                           y [batch, m * A], row stride ld_y
 * No mask, no bias, no dropout, no LayerNorm.
 *   Rounding.  X, the weights (through their bf16 images) and dY enter the products as bf16
 * (RNE where stored in fp32).  Accumulation is fp32 (MFMA).  Q, K, V are rounded once to
 * bf16.  S and the softmax are fp32 (exp, a true division by the sum).  P is rounded once to
 * bf16 before P V.  O + X Wres^T is added in fp32.  Y is rounded once when y_dtype is
 * MREC_BF16.  In the backward scale * dS, dQ, dK and dV are each rounded once to bf16 before
 * the product that consumes them; the softmax derivative uses the fp32 P.
 *   Weight images (bf16, built by the caller whenever a weight changes):
 *   w_fwd [mrec_autoint_image_rows(A) = 4 A][d_in]   rows [Wres | Wq | Wk | Wv]
 *   w_bwd [d_in][4 A]                                 its transpose
 * Without Wres its rows are zeros and has_res is 0.
 *   Backward (mrec_autoint_bwd: a data-gradient launch, a weight-gradient launch and the sum
 * of its partials).  y is the forward's output, an input here; dZ = dY * (Y > 0):
 *   dV_h = P_h^T dZ_h      dP_h = dZ_h V_h^T      dS_h = P_h * (dP_h - rowsum(dP_h * P_h))
 *   dQ_h = scale * dS_h K_h       dK_h = scale * dS_h^T Q_h
 *   dx   = dQ Wq + dK Wk + dV Wv + dZ Wres          rounded once into dx_dtype, overwritten
 *   dw   = sum over batch and fields of (dQ | dK | dV | dZ)^T X
 * dw is contiguous fp32 [4 (3 without Wres)][A][d_in] in the order q, k, v, res, overwritten.
 * Q, K, V, S and P are recomputed from x: nothing but x and y is kept between the directions.
 * workspace (16-byte aligned, mrec_autoint_bwd_workspace_size bytes) holds the transposed
 * (dZ | dQ | dK | dV) rows in bf16 and the weight gradient's per-workgroup fp32 partials.
 *   Determinism: no atomics; y and dx of a sample depend on that sample alone; dw is summed
 * over each workgroup's own samples in order, then over the workgroups in order.
 *   One description for both directions: the forward ignores dy, dx, dw, w_bwd and the
 * workspace.
 * Compiled shapes (mrec_autoint_supported): 2 <= n_fields <= 32, d_in in {8, 16, 32, 64}, A
 * in {16, 32, 64}, head_dim in {8, 16, 32} dividing A; x, y, dy, dx each MREC_F32 or
 * MREC_BF16 with 16-byte aligned rows.  batch = 0 launches nothing.  Never read or written:
 * columns past the stated widths, rows >= batch.  Anything else is MREC_EINVAL with
 * mrec_last_error() before any launch.
 */
typedef struct {
  const void *x;
  mrec_dtype x_dtype;
  int64_t ld_x;
  const void *w_fwd;
  int64_t ld_w_fwd;
  const void *w_bwd;
  int64_t ld_w_bwd;
  int32_t has_res;
  int64_t batch;
  int32_t n_fields;
  int32_t d_in;
  int32_t heads;
  int32_t head_dim;
  int32_t A;
  float scale;
  void *y; /* written by the forward, read by the backward */
  mrec_dtype y_dtype;
  int64_t ld_y;
  const void *dy;
  mrec_dtype dy_dtype;
  int64_t ld_dy;
  void *dx;
  mrec_dtype dx_dtype;
  int64_t ld_dx;
  float *dw;
  void *workspace;
  int64_t workspace_bytes;
} mrec_autoint_args;

int32_t mrec_autoint_supported(int32_t n_fields, int32_t d_in, int32_t heads, int32_t head_dim,
                               mrec_dtype x_dtype, mrec_dtype y_dtype);
int32_t mrec_autoint_image_rows(int32_t A); /* rows of w_fwd = columns of w_bwd */
int64_t mrec_autoint_bwd_workspace_size(int64_t batch, int32_t d_in, int32_t A);
mrec_status mrec_autoint_fwd(const mrec_autoint_args *args, mrec_stream stream);
mrec_status mrec_autoint_bwd(const mrec_autoint_args *args, mrec_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* MREC_H */
