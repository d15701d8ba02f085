/*
 * mmlrec.h -- C ABI of the MI355X-native MMLRec hot path (libmmlrec_hip.so).
 *
 * The reference (alipay/MMLRec) is pure Python/PyTorch and has no FFI of its own: the boundary it
 * exposes is the nn.Module contract (forward(X, domain_mask) in model/{sharedbottom,mmoe,ple,star,pepnet}.py
 * driven by BaseModel.fit, model/basemodel.py:261-313).  Everything below that contract is ATen.  This header
 * declares the entry points that replace those ATen call sites; each one cites the reference lines whose
 * arithmetic it takes over.  INTEGRATION.md shows the ctypes stub a reference maintainer would add.
 *
 * Conventions
 *   - plain C: raw device pointers, sizes, a hipStream_t passed as void*; no torch types.
 *   - every function returns MML_OK (0) or a negative error code and never throws; mml_last_error()
 *     returns a thread-local message for the last failure.
 *   - caller owns every buffer.  Nothing is allocated inside a call; kernels that need scratch take an
 *     explicit workspace pointer + size and a *_workspace_bytes() query tells how much they need.
 *   - descriptor arrays (mml_*_desc) live in HOST memory; they are copied into the kernel argument
 *     block, so no hidden H2D traffic and the calls are hipGraph-capturable.
 *   - all matrices are fp32 row-major with an explicit leading dimension (elements, not bytes).
 *   - re-entrant on different streams; no global state besides the thread-local error string.
 *   - device-side problems (an index outside its table) set bits in an optional int32 status word
 *     instead of trapping: bit 0 = index < 0, bit 1 = index >= vocab (nn.Embedding raises IndexError
 *     on CPU for these; the host wrapper turns a non-zero status into the same exception).
 */
#ifndef MMLREC_H
#define MMLREC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MML_OK 0
#define MML_ERR_ARG (-1)         /* bad argument (null pointer, size out of range, misaligned buffer) */
#define MML_ERR_HIP (-2)         /* a HIP runtime call failed; see mml_last_error() */
#define MML_ERR_UNSUPPORTED (-3) /* valid request the library does not implement */

#define MML_MAX_FIELDS 64   /* sparse fields per gather/scatter launch (more: call again with the next slice) */
#define MML_MAX_GROUP 16    /* GEMM problems per grouped launch */
#define MML_MAX_SRC 8       /* accumulated sources per dgrad output */
#define MML_MAX_EXPERTS 16  /* experts visible to one gate group */
#define MML_MAX_GATES 8     /* gates per gate group */
#define MML_MAX_HEADS 8     /* prediction heads per head launch */
#define MML_MAX_OPT_TENSORS 32
#define MML_AMAX_WORDS 8    /* words of one operand-magnitude slot (see "operand magnitudes" at the GEMM family) */
#define MML_MAX_AMAX 64     /* tensors per mml_amax_batch launch (16 until round 6: PepNet's 42 stable weights took three launches) */

typedef void* mml_stream_t; /* hipStream_t */

/* activation / derivative codes */
#define MML_ACT_NONE 0
#define MML_ACT_RELU 1
#define MML_ACT_SIGMOID 2
#define MML_ACT_SIGMOID2 3 /* 2*sigmoid(x): PepNet GateNN (model/pepnet.py:31-32) */

/* optimizer kinds: torch.optim defaults as used by BaseModel._get_optim (model/basemodel.py:569-584) */
#define MML_OPT_SGD 0
#define MML_OPT_ADAM 1
#define MML_OPT_ADAGRAD 2
#define MML_OPT_RMSPROP 3

int mml_version(void);
const char* mml_last_error(void);
/* out[0]=CU count, [1]=LDS bytes/CU, [2]=total HBM bytes, [3]=wavefront size, [4]=max clock kHz, [5]=gfx arch number */
int mml_device_caps(int device, int64_t* out6);
/* A HIP stream whose kernels may only run on compute units [cu_lo, cu_hi) of `device` (bit i of the queue's CU mask;
 * on gfx950 the driver deals mask bits round-robin over the 8 XCDs, so a contiguous range takes the same number of CUs
 * from every XCD).  Lets an HBM-bound stream (the dense table optimizer) and an MFMA-bound one (the weight-gradient
 * GEMMs) run side by side instead of alternating workgroup by workgroup.  mml_stream_destroy releases it. */
int mml_stream_create_cu_range(int device, int cu_lo, int cu_hi, mml_stream_t* stream_out);
int mml_stream_destroy(mml_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * K1  fused multi-field gather + concat.
 * Replaces BaseModel.input_from_feature_columns (model/basemodel.py:461-487: per field
 * nn.Embedding(X[:, c].long())) and combined_dnn_input (model/utils.py:434-446: cat + flatten + cat).
 *   out[b, f*E + e]   = tables[f][trunc(X[b, col[f]]) * E + e]     f < F, e < E   (bit-exact copy)
 *   out[b, F*E + j]   = X[b, dense_col0 + j]                       j < Nd
 * X carries indices as fp32 (model/basemodel.py:262, :476) -> exact below 2^24 rows.
 * tables/vocab/col are HOST arrays of length F (tables holds DEVICE pointers).
 * ---------------------------------------------------------------------------------------------- */
int mml_gather_fwd(const float* const* tables, const int64_t* vocab, const int32_t* col, int32_t F, int32_t E,
                   const float* X, int64_t ldX, int32_t dense_col0, int32_t Nd, int64_t B,
                   float* out, int64_t ldo, int32_t* status, mml_stream_t stream);
/* mml_gather_fwd that also leaves the magnitude of what it wrote: workgroup w stores the largest |value| of its part
 * of `out` to wg_max[w] (plain stores, no atomics; wg_max_len = mml_gather_wgmax_len(F, E, Nd, B) values, all of them
 * written by every call).  Feeding wg_max -- viewed as one row of floats -- to mml_amax_batch gives the magnitude slot of
 * `out` from a few KB instead of a pass over the whole output.  Needs E % 4 == 0, ldo % 4 == 0 and 16-byte aligned
 * tables and output (MML_ERR_ARG otherwise). */
int64_t mml_gather_wgmax_len(int32_t F, int32_t E, int32_t Nd, int64_t B);
/* Kernel symbol of the calling thread's most recent gather launch ("gather_vec4_kernel", "gather_lds_kernel" -- the
 * LDS-staged variant for tables of at most 128 rows, north_star's "LDS-staged index dedup", which runs when the
 * environment holds MMLREC_GATHER_LDS = n > 0 workgroups per CU at the time of the call and the launch neither marks rows
 * nor leaves workgroup maxima -- or "gather_scalar_kernel"); "" before the first one.  For tests / benchmark labels. */
const char* mml_gather_last_kernel(void);
int mml_gather_fwd_wgmax(const float* const* tables, const int64_t* vocab, const int32_t* col, int32_t F, int32_t E,
                         const float* X, int64_t ldX, int32_t dense_col0, int32_t Nd, int64_t B, float* out,
                         int64_t ldo, float* wg_max, int64_t wg_max_len, int32_t* status, mml_stream_t stream);
/* mml_gather_fwd that also marks every row it reads in row_marks (a byte per table row, layout and contract of
 * mml_scatter_bwd's row_marks): the split dense table update (mml_opt_tensor.skip_rows) gets the batch's row set from
 * the gather itself; mml_rows_compact then turns the marks into the `seen` bitmaps and the touched-row list
 * (touched[] = every marked or already-seen row, *touched_count = their number; the marks are cleared). */
int mml_gather_fwd_mark(const float* const* tables, const int64_t* vocab, const int32_t* col, int32_t F, int32_t E,
                        const float* X, int64_t ldX, int32_t dense_col0, int32_t Nd, int64_t B, float* out,
                        int64_t ldo, uint8_t* row_marks, int32_t* status, mml_stream_t stream);
int mml_rows_compact(uint32_t* const* seen, const int64_t* vocab, const int64_t* rowbase, int32_t F, int32_t* touched,
                     int32_t* touched_count, int32_t touched_cap, uint8_t* row_marks, mml_stream_t stream);
/* same with native int32 indices idx[b*ldi + f] (additive API for vocabularies >= 2^24);
 * dense values come from dense[b*ldd + j] (may be null when Nd == 0). */
int mml_gather_fwd_idx32(const float* const* tables, const int64_t* vocab, int32_t F, int32_t E,
                         const int32_t* idx, int64_t ldi, const float* dense, int64_t ldd, int32_t Nd, int64_t B,
                         float* out, int64_t ldo, int32_t* status, mml_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * K2  sparse row-scatter backward of K1.
 * Replaces aten::embedding_dense_backward triggered by sparse=False (model/basemodel.py:122,
 * model/utils.py:476):  grad_tables[f][idx[b,f], :] += dOut[b, f*E:(f+1)*E]  (duplicates accumulate).
 * grad_tables are dense [V_f, E] accumulators owned by the caller (zeroed by the caller, or kept zero
 * between steps by mml_opt_step_rows).  Duplicate rows inside a workgroup are pre-reduced in LDS before
 * one float atomic per (row, e) reaches HBM, so the result is order-dependent in the last bits.
 * If `touched` is non-null the first writer of a row (per-table bitmap `seen[f]`, V_f bits rounded up to
 * 32) appends the global row id rowbase[f] + idx to touched[0..cap) and bumps *touched_count: the compact row
 * list the sparse-row optimizer walks.  rowbase is a HOST array of F+1 int64 (exclusive prefix sum of vocab).
 * ---------------------------------------------------------------------------------------------- */
int mml_scatter_bwd(float* const* grad_tables, const int64_t* vocab, const int32_t* col, int32_t F, int32_t E,
                    const float* X, int64_t ldX, int64_t B, const float* dOut, int64_t ldo,
                    uint32_t* const* seen, const int64_t* rowbase, int32_t* touched, int32_t* touched_count,
                    int32_t touched_cap, uint8_t* row_marks, int32_t* status, mml_stream_t stream);
/* row_marks (optional, may be NULL): a DEVICE scratch map of 32 * sum_f ceil(V_f / 32) bytes, all-zero between calls
 * (field f owns the bytes from 32 * sum_{g<f} ceil(V_g / 32)).  With it the rows are marked by plain byte stores and
 * the list / bitmaps are rebuilt from the marks by a compaction pass (touched[] = every marked or already-seen row,
 * *touched_count = their number) instead of one same-address atomic per hot row: 350 us -> 30 us for the index-only
 * pass at B = 65 536 on the AliExpress-shaped tables.
 * row_marks WITHOUT a touched list (touched == NULL): the scatter only marks every row it adds to and leaves the bytes
 * set -- the consumer is mml_opt_step_dense with mml_opt_tensor.grad_marks, which skips the gradient read of unmarked
 * rows and clears the marks.  Needs the LDS-fold kernel (E in {4, 8, 16}, 16-byte aligned dOut, ldo % 4 == 0); other
 * shapes are rejected (MML_ERR_ARG) rather than served by a kernel that would leave the marks unset. */

/* Unique (field, row) list of a batch WITHOUT gradients: the scatter's LDS dedup run on the indices alone.  Appends
 * rowbase[f] + row for every distinct row of X[:, col[f]] to touched[] (first-seen order, `seen` bitmaps as above).
 * Used by the lazy-exact table optimizer, which must bring exactly these rows up to date BEFORE the gather reads
 * them. */
int mml_index_unique(const int64_t* vocab, const int32_t* col, int32_t F, int32_t E, const float* X, int64_t ldX,
                     int64_t B, uint32_t* const* seen, const int64_t* rowbase, int32_t* touched,
                     int32_t* touched_count, int32_t touched_cap, uint8_t* row_marks, int32_t* status,
                     mml_stream_t stream);

/* Deterministic form of mml_scatter_bwd ("mode: sorted" of SURVEY 8(b), without the sort): the same LDS fold, but
 * every addend is turned into 64-bit fixed point with ONE unit for the whole launch (taken from max |dOut|, which the call
 * measures into amax_slot: MML_AMAX_WORDS words) and the chunk sums are added to 64-bit integer row accumulators
 * acc64[f] ([V_f, E] int64, all zero between calls) with integer atomics; a second launch turns the totals of the
 * marked rows into fp32, adds them to grad_tables and zeroes them again.  Integer sums do not depend on the order of
 * the addends, so the result is BITWISE repeatable and independent of the order of the samples in the batch (a sorted
 * fp32 sum would still depend on it); accuracy: addends down to 2^-(62 - 24 - ceil(log2 B)) of the largest |dOut| are
 * summed exactly.  row_marks: the byte map of mml_scatter_bwd (required: the second launch walks it).  E in {4, 8, 16},
 * dOut 16-byte aligned.
 * flags (0 and 1 are the former clear_marks argument; any other bit than these three is MML_ERR_ARG):
 *   MML_SCATTER_DET_CLEAR_MARKS    the second launch clears the marks it finds; without it they stay set for
 *                                  mml_opt_tensor.grad_marks / mml_rows_compact.
 *   MML_SCATTER_DET_AMAX_SUPPLIED  amax_slot already holds the magnitude of dOut[0:B, 0:F*E] -- raised by the launch that
 *                                  wrote dOut (mml_gemm_dgrad_desc.amax_out) on a slot zeroed before it: the call issues
 *                                  neither mml_amax_reset nor mml_amax_batch.  Only the exponent of the largest word is
 *                                  used, so any producer that records the exact maximum of what it stored gives the bits
 *                                  the call's own pass gives.
 *   MML_SCATTER_DET_DEFER_TOTALS   no second launch: the row totals stay in acc64 and the marks stay set, and the caller
 *                                  owes ONE mml_opt_step_dense over every table with mml_opt_tensor.acc64 / acc_amax /
 *                                  acc_shift = acc64[f] / amax_slot / mml_scatter_det_shift(B), which adds the totals to
 *                                  the gradient it reads, zeroes them and clears the marks.  Not with CLEAR_MARKS. */
#define MML_SCATTER_DET_CLEAR_MARKS 1
#define MML_SCATTER_DET_AMAX_SUPPLIED 2
#define MML_SCATTER_DET_DEFER_TOTALS 4
int mml_scatter_bwd_det(float* const* grad_tables, const int64_t* vocab, const int32_t* col, int32_t F, int32_t E,
                        const float* X, int64_t ldX, int64_t B, const float* dOut, int64_t ldo, int64_t* const* acc64,
                        uint32_t* amax_slot, uint8_t* row_marks, int32_t flags, int32_t* status,
                        mml_stream_t stream);
/* log2 of the fixed-point scale mml_scatter_bwd_det uses for a batch of B samples (a function of B alone: 24 significand
 * bits + shift + ceil(log2 B) < 63, clamped to [4, 28]); a total t stands for t * 2^(emax - 150 - shift), emax = the
 * exponent field of the slot's largest word clamped to [1, 254]. */
int32_t mml_scatter_det_shift(int64_t B);
/* Native-index variants (int32 idx[b*ldi + f], fields in array order): vocabularies >= 2^24 and the
 * owner side of row-sharded tables, which sees lookups as keys into its flat row space (F = 1). */
int mml_scatter_bwd_idx32(float* const* grad_tables, const int64_t* vocab, int32_t F, int32_t E, const int32_t* idx,
                          int64_t ldi, int64_t B, const float* dOut, int64_t ldo, uint32_t* const* seen,
                          const int64_t* rowbase, int32_t* touched, int32_t* touched_count, int32_t touched_cap,
                          uint8_t* row_marks, int32_t* status, mml_stream_t stream);
int mml_index_unique_idx32(const int64_t* vocab, int32_t F, int32_t E, const int32_t* idx, int64_t ldi, int64_t B,
                           uint32_t* const* seen, const int64_t* rowbase, int32_t* touched, int32_t* touched_count,
                           int32_t touched_cap, uint8_t* row_marks, int32_t* status, mml_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * K1p / K2p  multi-valued (pooled) sparse features beside the single-valued ones.
 * Replaces, for a schema with VarLenSparseFeat columns, BaseModel.input_from_feature_columns
 * (model/basemodel.py:461-487), varlen_embedding_lookup (model/utils.py:520-533: nn.Embedding over the maxlen id
 * columns), get_varlen_pooling_list (model/utils.py:449-463: the mask from `ids != 0` or from the length column),
 * SequencePoolingLayer (model/utils.py:258-326: sum / mean / max over the positions) and combined_dnn_input
 * (model/utils.py:434-446), and their autograd backward.
 *
 * The descriptor names every TABLE once and every field, single-valued or pooled, names its table by index: an item
 * id column and a history of item ids share one table, one `seen` bitmap and one mark range.  All arrays are HOST
 * arrays; table[] holds DEVICE pointers ([vocab, E] fp32: the embedding tables for the gather, the gradient
 * accumulators for the scatter, unused by mml_index_unique_pool).
 * Caps: n_tables <= MML_MAX_FIELDS, n_single + n_pooled <= MML_MAX_FIELDS, n_pooled <= MML_MAX_POOLED,
 * 1 <= p_maxlen <= MML_POOL_MAX_LEN, E in {4, 8, 16}, vocab < 2^31; 16-byte aligned tables, out and dOut with
 * ldo % 4 == 0.  Anything else returns MML_ERR_ARG.
 *
 * Layout of out / dOut (the reference's dnn_input): [ single-valued blocks in array order | pooled blocks in array
 * order | Nd dense columns ], every block E wide.
 * Pooled field p owns the X columns [p_col0, p_col0 + p_maxlen) (ids as fp32, truncated toward zero).  Position t is
 * VALID iff  p_len_col <  0 (mask mode):   trunc(X[b, p_col0 + t]) != 0            (id 0 is padding, anywhere)
 *            p_len_col >= 0 (length mode): t < min(max(trunc(X[b, p_len_col]), 0), p_maxlen)   (id 0 is a row)
 *   MML_POOL_SUM   out = sum over the valid t of row_t                   (fp32, tree order)
 *   MML_POOL_MEAN  out = that sum / ((float)n_valid + 1e-8f)             (n_valid = 0 gives 0)
 *   MML_POOL_MAX   out = max over ALL t of (valid_t ? row_t : row_t - 1e9f); the first (lowest t) position that
 *                  attains it is stored per element in argmax[b * ldarg + p * E + e] (one byte; ldarg >= n_pooled * E,
 *                  ldarg % 4 == 0; argmax may be NULL when no field uses MML_POOL_MAX)
 * Indices are validated through `status` (bits of mml_gather_fwd) at VALID positions only; the id of a padded
 * position is clamped into the table before it is used as an address.
 * ---------------------------------------------------------------------------------------------- */
#define MML_MAX_POOLED 16
#define MML_POOL_MAX_LEN 256
#define MML_POOL_SUM 0
#define MML_POOL_MEAN 1
#define MML_POOL_MAX 2
typedef struct mml_pool_desc {
  int32_t n_tables, E, n_single, n_pooled;
  float* table[MML_MAX_FIELDS];
  int64_t vocab[MML_MAX_FIELDS];
  int32_t s_col[MML_MAX_FIELDS];   /* single-valued field f: its X column ... */
  int32_t s_table[MML_MAX_FIELDS]; /* ... and its table index */
  int32_t p_col0[MML_MAX_POOLED], p_maxlen[MML_MAX_POOLED], p_len_col[MML_MAX_POOLED];
  int32_t p_combiner[MML_MAX_POOLED], p_table[MML_MAX_POOLED];
} mml_pool_desc;
/* K1p: ONE launch writes the whole dnn_input.  Single-valued blocks and dense columns are bit-exact copies (the
 * contract of mml_gather_fwd).  wg_max (optional): workgroup w stores the largest |value| it wrote to wg_max[w]
 * (contract of mml_gather_fwd_wgmax); wg_max_len must equal mml_gather_pool_wgmax_len(). */
int64_t mml_gather_pool_wgmax_len(const mml_pool_desc* d, int32_t Nd, int64_t B);
int mml_gather_pool_fwd(const mml_pool_desc* d, const float* X, int64_t ldX, int32_t dense_col0, int32_t Nd, int64_t B,
                        float* out, int64_t ldo, uint8_t* argmax, int64_t ldarg, float* wg_max, int64_t wg_max_len,
                        int32_t* status, mml_stream_t stream);
/* K2p: ONE launch adds the table gradients of every field: a single-valued field adds dOut[b, block] to its row,
 * a pooled field adds to the row of every VALID position  dOut (sum),  dOut / ((float)n_valid + 1e-8f) (mean),  or
 * dOut[e] where argmax[e] == t and 0 elsewhere (max; argmax as the gather left it).  Padded positions add nothing
 * and their row is not touched.  Duplicates (inside a sequence, across samples, across the fields of one table) are
 * folded in LDS in 64-bit fixed point in front of the float atomics, as in mml_scatter_bwd.
 * Bookkeeping per TABLE under the contracts of mml_scatter_bwd: seen[n_tables] bitmaps, rowbase[n_tables + 1],
 * touched / touched_count / touched_cap, row_marks (32 * sum_t ceil(V_t / 32) bytes, table t from
 * 32 * sum_{u<t} ceil(V_u / 32)), with or without a touched list.  A row reached through several fields is listed
 * once.  One difference from mml_scatter_bwd: the pool entry points ALWAYS rebuild the touched list by compaction
 * (mml_rows_compact over the tables), with or without a mark map -- *touched_count is reset and touched[] holds every
 * row whose bit is set in `seen` afterwards, rows of earlier calls included until the caller clears the bitmaps; no
 * form appends to an existing list.
 * An out-of-range id at a valid position (status bit set) is read as the clamped row by the gather and counts in
 * n_valid there; the scatter skips it and, in mask mode, does not count it: results of a batch whose status word is
 * set are not defined beyond "no address outside the tables is touched". */
int mml_scatter_pool_bwd(const mml_pool_desc* d, const float* X, int64_t ldX, int64_t B, const float* dOut,
                         int64_t ldo, const uint8_t* argmax, int64_t ldarg, uint32_t* const* seen,
                         const int64_t* rowbase, int32_t* touched, int32_t* touched_count, int32_t touched_cap,
                         uint8_t* row_marks, int32_t* status, mml_stream_t stream);
/* Deterministic form of K2p (what mml_scatter_bwd_det is to mml_scatter_bwd): the same launch, the same validity rules,
 * mean count, argmax routing and status reporting, but bitwise repeatable and independent of the order of the samples.
 *   addends   what K2p adds: dOut[b, block] (single-valued, sum), dOut / ((float)n_valid + 1e-8f) (mean: ONE fp32
 *             division, then the conversion) or dOut[e] where argmax[e] == t (max).  |addend| <= max |dOut|: the divisor
 *             of a valid position is >= 1.
 *   unit      2^(emax - 150 - shift), emax = the exponent field of the largest word of amax_slot (the magnitude of
 *             dOut[0:B, 0:(n_single + n_pooled) * E], measured by the call unless supplied) clamped to [1, 254], shift =
 *             mml_scatter_pool_det_shift(d, B).  Every addend is rounded to the unit ONCE (to nearest); the chunk sums
 *             in LDS and the row totals use the same unit, so every total is an exact integer sum of the rounded addends.
 *   headroom  row r of table tb can receive B * L_tb addends, L_tb = the single-valued fields on tb + the sum of maxlen
 *             over the pooled fields on tb: 24 significand bits + shift + ceil(log2(B * max_tb L_tb)) < 63 with
 *             shift = min(28, 62 - 24 - ceil(log2(B * max_tb L_tb))).  Where that leaves shift < 4 the rule returns a
 *             negative value and the entry point MML_ERR_ARG (B * max_tb L_tb > 2^34).  For a schema without pooled
 *             fields and one field per table the rule is mml_scatter_det_shift(B).
 *   totals    acc64[t]: int64 [V_t, E] per TABLE (n_tables pointers, all zero between calls); fields that share a table
 *             add to the same totals, so shared tables are allowed.  row_marks (required): the per-table byte map of
 *             mml_scatter_pool_bwd.  The second launch turns the totals of the marked rows into fp32, adds them to
 *             d->table[t] and zeroes them.  Inf / NaN addends are not folded: they reach d->table[t] as float atomics.
 *   flags     MML_SCATTER_DET_CLEAR_MARKS / _AMAX_SUPPLIED / _DEFER_TOTALS with the meaning and the exclusions of
 *             mml_scatter_bwd_det (deferred totals: acc_shift = mml_scatter_pool_det_shift(d, B)); any other bit is
 *             MML_ERR_ARG.
 * The descriptor checks are those of mml_scatter_pool_bwd; acc64, every acc64[t], amax_slot and row_marks are required. */
int32_t mml_scatter_pool_det_shift(const mml_pool_desc* d, int64_t B);
int mml_scatter_pool_bwd_det(const mml_pool_desc* d, const float* X, int64_t ldX, int64_t B, const float* dOut,
                             int64_t ldo, const uint8_t* argmax, int64_t ldarg, int64_t* const* acc64,
                             uint32_t* amax_slot, uint8_t* row_marks, int32_t flags, int32_t* status,
                             mml_stream_t stream);
/* The distinct VALID rows of a batch without gradients (the counterpart of mml_index_unique, same outputs, per
 * table): what the lazy-exact table optimizer brings up to date before the gather reads it. */
int mml_index_unique_pool(const mml_pool_desc* d, const float* X, int64_t ldX, int64_t B, uint32_t* const* seen,
                          const int64_t* rowbase, int32_t* touched, int32_t* touched_count, int32_t touched_cap,
                          uint8_t* row_marks, int32_t* status, mml_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Row-wise sharded tables (replaces the reference's dead --is_parallel stub, main.py:81-83,
 * model/basemodel.py:235-238).  Row r of field f lives on rank (r + f) mod world at local row r / world; a rank keeps
 * its F shards back to back in one flat [R, E] buffer and a lookup travels as the int32 key keybase[f] + r / world.
 *   mml_route_count  counters[0..world) = lookups of the batch bound for each owner (counters[world..2*world) is
 *                    cleared for mml_route_place); indices are validated / clamped like mml_gather_fwd (status bits).
 *   mml_route_place  send_keys[B*F] = keys grouped by owner (owner segments in rank order: the send layout of ONE
 *                    all-to-all over all fields), pos[b*F + f] = position of (b, f)'s key in send_keys.  Needs the
 *                    counters of mml_route_count on the same batch.  Order inside an owner segment is unspecified.
 *   mml_rows_permute dst[pos[b*F+f], :] = src[b, f*E:(f+1)*E]: packs d(dnn_input) into the send order of the gradient
 *                    exchange (the inverse direction is mml_gather_fwd_idx32 on the received row block).
 *   mml_shard_rows   shard[l, :] = table[l*world + first, :] (to_table = 0; rows past the table end are zero) or the
 *                    inverse copy (to_table = 1); first = (rank - f) mod world.
 * X / idx: exactly one is non-null (fp32-encoded indices with column map col[], or native int32 [B, ldi]).
 * col, vocab, keybase are HOST arrays of F entries; counters, send_keys, pos, status are DEVICE buffers.
 * ---------------------------------------------------------------------------------------------- */
int mml_route_count(const float* X, int64_t ldX, const int32_t* idx, int64_t ldi, const int32_t* col,
                    const int64_t* vocab, int32_t F, int64_t B, int32_t world, int32_t* counters, int32_t* status,
                    mml_stream_t stream);
int mml_route_place(const float* X, int64_t ldX, const int32_t* idx, int64_t ldi, const int32_t* col,
                    const int64_t* vocab, const int64_t* keybase, int32_t F, int64_t B, int32_t world,
                    int32_t* counters, int32_t* send_keys, int32_t* pos, int32_t* status, mml_stream_t stream);
int mml_rows_permute(const float* src, int64_t lds, const int32_t* pos, int32_t F, int32_t E, int64_t B, float* dst,
                     mml_stream_t stream);
int mml_shard_rows(float* table, int64_t V, float* shard, int64_t rows_local, int32_t E, int32_t world, int32_t first,
                   int32_t to_table, mml_stream_t stream);
/* Requester-side de-duplication: route the batch's DISTINCT rows (the touched list of mml_index_unique: global row ids
 * rowbase[f] + r, *count of them on the device, capacity cap) instead of its B*F lookups -- under Zipf a 65 536-sample
 * AliExpress-shaped batch holds 209 k distinct rows against 1.97 M lookups.
 *   mml_route_list_count / _place   as mml_route_count / _place, over the list; _place also writes
 *                                   slot_of[global row id] = position of the row's key in send_keys
 *   mml_lookup_slots                pos[b*F + f] = slot_of[rowbase[f] + trunc(X[b, col[f]])]  (indices validated / clamped)
 *   mml_rows_clear                  clears the `seen` words of the listed rows (requester-side bitmaps)
 * slot_of is a DEVICE int32 array of rowbase[F] entries (only the listed rows are written / read). */
int mml_route_list_count(const int32_t* list, const int32_t* count, int32_t cap, const int64_t* vocab,
                         const int64_t* rowbase, int32_t F, int32_t world, int32_t* counters, mml_stream_t stream);
int mml_route_list_place(const int32_t* list, const int32_t* count, int32_t cap, const int64_t* vocab,
                         const int64_t* rowbase, const int64_t* keybase, int32_t F, int32_t world, int32_t* counters,
                         int32_t* send_keys, int32_t* slot_of, mml_stream_t stream);
int mml_lookup_slots(const float* X, int64_t ldX, const int32_t* col, const int64_t* vocab, const int64_t* rowbase,
                     int32_t F, int64_t B, const int32_t* slot_of, int32_t* pos, int32_t* status, mml_stream_t stream);
int mml_rows_clear(const int32_t* list, const int32_t* count, int32_t cap, const int64_t* rowbase,
                   uint32_t* const* seen, int32_t F, mml_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * K3  grouped GEMM family on the fp32 MFMA pipe (v_mfma_f32_32x32x2_f32: exact fp32 products and sums).
 * Replaces nn.Linear + activation inside DNN.forward (model/utils.py:146-161: addmm, relu_) and the
 * autograd mm/mm backward pair of each layer.
 * ---------------------------------------------------------------------------------------------- */
/* Arithmetic of the GEMM family (process-wide):
 *   0 = fp32 MFMA on every launch (v_mfma_f32_32x32x2_f32: bitwise an fmaf chain);
 *   4 = auto (DEFAULT): fp32-equivalent.  Where it is faster, every fp32 operand value is cut in registers into three
 *       bf16 planes h + m + l == x (exact mantissa slices) and a 16-k product block costs six
 *       v_mfma_f32_32x32x16_bf16 (hh, hm, mh, mm, hl, lh; the dropped terms are <= 2^-24 |a b|) with fp32
 *       accumulation.  Max-norm error against float64 equals the fp32 MFMA's (4.7e-7 vs 4.3e-7 on a
 *       8192 x 256 x 240 product, tools/bench_gemm.py); the other launches use the fp32 MFMA;
 *       When every operand of a launch comes with its magnitude (the amax fields of the descriptors below), auto runs
 *       the TWO-PLANE fp16 form instead: each operand is scaled by a power of two that puts its largest magnitude below
 *       2^15, cut into h = rne16(x s), l = rne16(x s - h) (x s = h + l to 22-23 significant bits), a 16-k block costs
 *       three v_mfma_f32_32x32x16_f16 (hh, hl, lh) and the fp32 accumulators are scaled back exactly in the epilogue.
 *       Max-norm error against float64 3.4e-7 (three bf16 planes 4.7e-7, fp32 MFMA 4.3e-7), 25-30 % faster;
 *   2 = same as auto;
 *   3 = the three-plane bf16 form on every launch of the LDS-DMA kernel (magnitudes ignored);
 *   1 = REDUCED precision, opt-in: operands rounded to bf16 in registers, one v_mfma_f32_32x32x16_bf16 per 16-k block,
 *       fp32 accumulation (~3e-3 relative per product; not covered by the 1e-4 parity contract).
 * Environment MMLREC_GEMM_MODE overrides the default. */
int mml_gemm_set_mode(int32_t mode);
int mml_gemm_get_mode(void);
/* Activation-stationary forward (csrc/gemm_panel.hip).  A forward launch whose problems all read ONE input A [M, K] (the
 * first DNN layer of every expert / gate tower: reference model/mmoe.py:69-79) with K in {160, 208, 240}, M >= 8 192 and
 * M % 128 == 0, N % 64 == 0 (an even number of 64-column half tiles over the launch), nn.Linear weights with pre-cut
 * planes, the magnitude of A, activation relu, 16-byte aligned operands, and relu sign masks on all problems or on
 * none, is served by a persistent workgroup per 128-row block that keeps the block's fp16 planes as MFMA fragments in
 * registers and sweeps every N-tile past them (bitwise the results of the tile kernel).  on = 0 switches it off
 * (process-wide; default on; environment MMLREC_GEMM_PANEL=0 does the same). */
int mml_gemm_set_panel(int32_t on);
/* Weight-stationary streaming GEMM (csrc/gemm_ws.hip).  A forward launch whose problems ALL have K % 64 == 0 or K % 80 == 0, N in {64,
 * 128, 256}, N K <= 32 768 (the two fp16 planes of the weight fit 128 KiB of LDS), one M >= 8 192, pre-cut planes (either
 * weight layout), the magnitude of A and activation relu, none, sigmoid or 2 sigmoid -- and an input-gradient launch of
 * single-source problems with K in {64, 128, 256} output columns, N % 64 == 0 or N % 80 == 0, N K <= 32 768, activation none or relu by sign
 * mask -- is served by persistent workgroups that keep one problem's weight planes in LDS while their waves stream 32-row
 * blocks of the batch past them (second expert layers, towers, PepNet's and STAR's layers: reference model/mmoe.py:69-119,
 * model/pepnet.py:64-78, model/utils.py:171-218); problems of different widths in one call become one kernel launch per
 * width.  Bitwise the results of the tile kernel.  on = 0 switches it off (default on; environment MMLREC_GEMM_WS=0 does
 * the same). */
int mml_gemm_set_ws(int32_t on);
/* Weight gradients cut once per workgroup (csrc/gemm_nt.hip).  A weight-gradient launch of <= 16 (MML_MAX_GROUP) problems in nn.Linear
 * layout that all carry both operand magnitudes, with M % 32 == 0, M >= 16 384, N % 32 == 0, K % 4 == 0 and 16-byte
 * aligned operand rows (the DNN layers of a large batch: reference model/utils.py:146-161, autograd's mm backward) is
 * served by workgroups that own a 128 x 128 tile of dW for a slab of the batch: the rows of both operands are cut into
 * their fp16 planes ONCE, stored to LDS as they lie in memory, and the MFMA fragments -- consecutive batch rows of a column
 * -- are read with the transposing LDS read ds_read_b64_tr_b16; partial tiles go to the same workspace, summed in slab order.
 * Same products and fp32 accumulation as the tile kernel, another summation order (not bitwise equal to it; bitwise
 * repeatable).  on = 0 never, 1 (default) every qualifying launch, 2 launches of at least 16 output tiles, 3 a measured
 * lab variant (the dC fragments loaded straight from global memory, half the LDS traffic: 19-21 % slower, kept for the
 * record); environment MMLREC_GEMM_NT sets the same (csrc/gemm_nt.hip holds the numbers: AE-30 step 1.68 -> 1.60 ms on
 * one box). */
int mml_gemm_set_nt(int32_t on);
/* Kernel symbol (as rocprofv3 prints it, without the mml:: prefix) of the calling thread's most recent GEMM launch;
 * "" before the first one.  For profilers / benchmark labels. */
const char* mml_gemm_last_kernel(void);
/* Unused dynamic LDS requested by the weight-gradient launches (process-wide, default 0).  A trainer that runs the
 * wgrad GEMMs on a side stream next to an HBM-bound kernel (the dense table optimizer) sets ~17 KiB so that only three
 * wgrad workgroups fit a CU and the other kernel's waves can co-reside. */
int mml_gemm_set_wgrad_lds_pad(int32_t bytes);

/* Operand magnitudes.  A magnitude slot is MML_AMAX_WORDS consecutive uint32 words on the device; its value is the
 * LARGEST of them, read as the bit pattern of a non-negative float: an upper bound of max |x| over a tensor (0 = the
 * tensor is all zero).  Producers raise a slot with atomic max on any of its words (mml_amax_batch; the GEMM launches
 * through amax_out: the magnitude of what they stored), nobody lowers it: mml_amax_reset zeroes slots at the start of a
 * step.  A GEMM launch whose descriptors all carry the magnitudes of BOTH operands may run the two-plane fp16
 * arithmetic (mml_gemm_set_mode); a stale-high bound costs precision only at 2^-39 of the bound, a too-LOW bound
 * overflows fp16 -- so a slot must cover everything the tensor holds when the GEMM runs. */
typedef struct {
  const float* x;   /* [rows, cols], row pitch ld */
  int64_t rows, ld;
  int32_t cols, pad_;
  uint32_t* slot;   /* MML_AMAX_WORDS words */
} mml_amax_desc;
int mml_amax_batch(const mml_amax_desc* descs, int32_t n, mml_stream_t stream);
int mml_amax_reset(uint32_t* slots, int64_t n_slots, mml_stream_t stream);

typedef struct {
  const float* A;    /* [M, K] input activations                                  */
  const float* W;    /* [N, K] nn.Linear weight layout (model/utils.py:130)        */
  const float* bias; /* [N] or NULL                                                */
  float* C;          /* [M, N] = act(A W^T + bias)                                 */
  int64_t lda, ldw, ldc;
  int32_t M, N, K;
  int32_t act;       /* MML_ACT_*                                                  */
  int32_t w_kn;      /* 0: W is [N,K] (nn.Linear); 1: W is [K,N] (STAR SharedSpecificLinear layout, model/utils.py:171) */
  int32_t pad_;
  /* Optional (training): when non-NULL and act == MML_ACT_RELU, bit (c & 31) of relu_mask[r * ldmask + (c >> 5)] is
   * set to (C[r][c] > 0) -- 1 bit per output instead of the 4 bytes mml_gemm_grouped_dgrad would otherwise re-read
   * to apply relu'.  ldmask >= ceil(N / 32) words per row. */
  uint32_t* relu_mask;
  int64_t ldmask;
  /* Optional operand magnitudes (see above): of A, of W; amax_out receives the magnitude of C. */
  const uint32_t* amax_a;
  const uint32_t* amax_w;
  uint32_t* amax_out;
  /* Optional pre-cut weight (mml_gemm_planes_cut, layout MML_PLANES_ROWS for w_kn = 0): the two fp16 planes of W in a
   * buffer of W's own shape and pitch, and the exponent they were scaled with.  When every problem of a launch that runs
   * the two-plane arithmetic carries them, the kernel reads the planes instead of cutting W's fragments (same bits). */
  const uint32_t* w_planes;
  const int32_t* w_kexp;
  /* K7, optional (PepNet: x = h (.) GateNN(.), reference model/pepnet.py:31-32, :72-78, :139-140): with mul != NULL the
   * launch ALSO stores prod[r][c] = C[r][c] * mul[r][c] -- the gated layer input leaves the gate network's last Linear
   * (act = MML_ACT_SIGMOID2) without a pass of its own over memory.  mul, prod: [M, N] at pitches ldmul / ldprod,
   * 16-byte aligned, N % 4 == 0, C 16-byte aligned too; amax_prod receives the magnitude of prod.  Only on the LDS-DMA
   * kernel (K % 16 == 0, aligned operands): other shapes return MML_ERR_UNSUPPORTED. */
  const float* mul;
  float* prod;
  int64_t ldmul, ldprod;
  uint32_t* amax_prod;
} mml_gemm_fwd_desc;
int mml_gemm_grouped_fwd(const mml_gemm_fwd_desc* descs, int32_t n, mml_stream_t stream);
/* SURVEY 8(b) name of the K7 forward: mml_gemm_grouped_fwd restricted to descriptors that carry mul / prod. */
int mml_pep_gate_fwd(const mml_gemm_fwd_desc* descs, int32_t n, mml_stream_t stream);


typedef struct {
  float* dA;           /* [M, K] = sum_s dC_s W_s  (then * act'(Y) if act != NONE)            */
  const float* Y;      /* [M, K] forward OUTPUT of the layer that produced A (relu/sigmoid derivative source) or NULL */
  int64_t ldda, ldy;
  int32_t M, K;
  int32_t act;         /* activation whose derivative is applied in the epilogue             */
  int32_t n_src;
  int32_t accumulate;  /* 1: dA += result (after the derivative), 0: overwrite                */
  int32_t pad_;
  const float* dC[MML_MAX_SRC]; /* [M, N_s] gradients w.r.t. the pre-activation outputs      */
  const float* W[MML_MAX_SRC];  /* [N_s, K] (w_kn=0) or [K, N_s] (w_kn=1)                     */
  int64_t lddc[MML_MAX_SRC], ldw[MML_MAX_SRC];
  int32_t N[MML_MAX_SRC];
  int32_t w_kn[MML_MAX_SRC];
  /* Optional: the sign mask mml_gemm_grouped_fwd wrote for Y (act must be MML_ACT_RELU); used instead of Y. */
  const uint32_t* relu_mask;
  int64_t ldmask;
  /* Optional operand magnitudes: of dC[s] and W[s] for every source; amax_out receives the magnitude of dA as stored
   * (after the derivative and the accumulation). */
  const uint32_t* amax_dc[MML_MAX_SRC];
  const uint32_t* amax_w[MML_MAX_SRC];
  uint32_t* amax_out;
  /* Optional pre-cut weights of the sources (mml_gemm_planes_cut, layout MML_PLANES_COLS for w_kn = 0), all sources of
   * a problem cut as ONE group (one common exponent): honoured when every source of every problem of the launch has them. */
  const uint32_t* w_planes[MML_MAX_SRC];
  const int32_t* w_kexp[MML_MAX_SRC];
  /* K7 backward, optional ("gate mode", gate_h != NULL): the problem's input is a product x = h (.) g; the input gradient
   * v = sum_s dC_s W_s is NOT stored, the epilogue forms the gradients of the two factors from it:
   *     d_h (+)= v * g * act_h'(h)          d_g (+)= v * h * act_g'(g)
   * act_h / act_g: the activations that PRODUCED h / g (derivative from the outputs h, g; MML_ACT_NONE: factor 1), acc_h /
   * acc_g: 1 = add to what d_h / d_g hold.  dA, Y, act, accumulate, relu_mask and amax_out are ignored.  gate_h, gate_g,
   * d_h, d_g: [M, K] at pitches ld_h, ld_g, ld_dh, ld_dg, 16-byte aligned, K % 4 == 0; amax_dh / amax_dg receive the
   * magnitudes of what was stored.  Only on the LDS-DMA kernel, like mul / prod of the forward. */
  const float* gate_h;
  const float* gate_g;
  float* d_h;
  float* d_g;
  int64_t ld_h, ld_g, ld_dh, ld_dg;
  int32_t act_h, act_g, acc_h, acc_g;
  uint32_t* amax_dh;
  uint32_t* amax_dg;
} mml_gemm_dgrad_desc;
int mml_gemm_grouped_dgrad(const mml_gemm_dgrad_desc* descs, int32_t n, mml_stream_t stream);
/* SURVEY 8(b) name of the K7 backward: mml_gemm_grouped_dgrad restricted to gate-mode descriptors. */
int mml_pep_gate_bwd(const mml_gemm_dgrad_desc* descs, int32_t n, mml_stream_t stream);

/* Pre-cut weights for the two-plane fp16 arithmetic.  The GEMM kernels cut every fp32 operand fragment into its planes
 * h = rne16(x 2^k), l = rne16(x 2^k - h) in registers, once per wave that reads it; a weight matrix is read by every row
 * tile of the batch, so it can be cut ONCE per step instead: `planes` has W's shape and pitch and holds, per aligned
 * block of 16 values along the reduction, the 32 bytes of h and the 32 bytes of l in the order the kernel's fragment
 * reads deliver them (so the planes travel through the same LDS image as the floats would).
 *   MML_PLANES_ROWS: the reduction runs along a ROW of W ([N, K] read by the forward: K % 16 == 0, or any K with ldp;
 *                    a [K, N] matrix (w_kn = 1) read by the input gradient);
 *   MML_PLANES_COLS: the reduction runs down the ROWS of W ([N, K] read by the input gradient: N % 16 == 0; a [K, N]
 *                    matrix read by the forward).
 * k = the largest exponent that keeps every |w| 2^k below 2^15 for the LARGEST of the n_amax magnitude slots given
 * (the weights that feed one input-gradient problem share their exponent); it is written to *kexp.  Bit-identical to
 * the in-kernel cut with the same magnitudes. */
#define MML_PLANES_ROWS 0
#define MML_PLANES_COLS 1
#define MML_MAX_PLANES 64
typedef struct {
  const float* W;     /* [rows, cols], row pitch ld (floats) */
  uint32_t* planes;   /* [rows, cols] 4-byte words at row pitch ldp */
  int64_t rows, ld;
  int32_t cols, layout;
  int32_t n_amax, pad_;
  const uint32_t* amax[MML_MAX_SRC];
  int32_t* kexp;
  /* Row pitch of `planes` in words; 0 = ld.  A wider pitch serves the zero-padded operand a GEMM reads when the
   * reduction extent is not a multiple of 16 (K0 = 303 -> 304): with MML_PLANES_ROWS, cols may then be ANY length and
   * the last, partial block is cut as if the missing columns were zero (ldp >= cols rounded up to 16; the words of the
   * missing columns are written as zero planes); with MML_PLANES_COLS the columns beyond `cols` are not touched (the
   * caller zeroes the buffer once). */
  int64_t ldp;
  /* K6, optional (STAR, reference model/utils.py:214-218: the layer's weight is W_specific (.) W_shared): with W2 != NULL
   * the planes are cut from the element-wise PRODUCT W[r][c] * W2[r][c] (W2: same shape, pitch ld2) -- the derived weight
   * reaches the GEMMs pre-cut without ever being read back.  The magnitude bound of the product is the product of the
   * factors' bounds: amax[0 .. n_amax) belong to the W factors of the group, amax[n_amax .. 2 n_amax) to their W2
   * factors (2 n_amax <= MML_MAX_SRC). */
  const float* W2;
  int64_t ld2;
} mml_planes_desc;
int mml_gemm_planes_cut(const mml_planes_desc* descs, int32_t n, mml_stream_t stream);
/* SURVEY 8(b) names of K6: the grouped forward / input-gradient GEMMs restricted to layers in STAR's [K, N] weight layout
 * (w_kn = 1) that carry pre-cut planes of the derived weight (mml_gemm_planes_cut with W2; layout MML_PLANES_COLS for the
 * forward -- the reduction runs down the rows of a [K, N] matrix --, MML_PLANES_ROWS for the input gradient). */
int mml_star_linear_fwd(const mml_gemm_fwd_desc* descs, int32_t n, mml_stream_t stream);
int mml_star_linear_bwd(const mml_gemm_dgrad_desc* descs, int32_t n, mml_stream_t stream);

typedef struct {
  const float* dC;  /* [M, N] gradient w.r.t. pre-activation output */
  const float* A;   /* [M, K] layer input                            */
  float* dW;        /* [N, K] (w_kn=0) or [K, N] (w_kn=1) = dC^T A   */
  float* dbias;     /* [N] = column sums of dC, or NULL              */
  int64_t lddc, lda, lddw;
  int32_t M, N, K;
  int32_t accumulate; /* 1: dW/dbias += ; 0: overwrite               */
  int32_t w_kn;
  int32_t pad_;
  /* Optional operand magnitudes of dC and A. */
  const uint32_t* amax_dc;
  const uint32_t* amax_a;
} mml_gemm_wgrad_desc;
/* The reduction over the batch is split across workgroups; partial tiles go to `workspace` and are
 * summed in a fixed order by a second kernel (bitwise reproducible). */
int64_t mml_gemm_grouped_wgrad_workspace_bytes(const mml_gemm_wgrad_desc* descs, int32_t n);
int mml_gemm_grouped_wgrad(const mml_gemm_wgrad_desc* descs, int32_t n, void* workspace, int64_t workspace_bytes,
                           mml_stream_t stream);
/* The same in two launches: phase 1 writes the per-chunk partial products to the workspace, phase 2 reduces them into
 * dW / dbias (phase 0 = both, as mml_gemm_grouped_wgrad).  A trainer that runs several weight-gradient GEMMs next to
 * an HBM-bound kernel issues all partials first and the (small, bandwidth-hungry) reductions last; each call then
 * needs its own workspace. */
int mml_gemm_grouped_wgrad_phase(const mml_gemm_wgrad_desc* descs, int32_t n, void* workspace,
                                 int64_t workspace_bytes, int32_t phase, mml_stream_t stream);
/* 1 when ONE weight-gradient problem satisfies every per-problem condition of the cut-once weight-gradient kernel
 * (mml_gemm_set_nt, csrc/gemm_nt.hip: layout, both magnitudes, M, N, K, alignment and row pitches), else 0.  A launch is
 * served when all of its problems are, they share M and there are at most 48 of them: a caller that groups problems into
 * launches (engine.Plan.merge_wgrad) asks here, so that its grouping and the library's decision cannot drift apart.  No GPU
 * work, no error text. */
int mml_gemm_nt_serves(const mml_gemm_wgrad_desc* desc);
/* 1 when mml_gemm_grouped_dgrad(desc, n) would run the output-stationary input-gradient kernel (csrc/gemm_os.hip:
 * gemm_os_kernel) on these descriptors, else 0: the GEMM mode is auto / two-plane, MMLREC_GEMM_OS is not 0 (read on every
 * call), n == 1, and the problem meets every condition of that kernel (plain epilogue, 2 .. MML_MAX_SRC nn.Linear-layout
 * sources with pre-cut planes of ONE exponent word and their gradients' magnitudes, M >= 16384, 192 <= K <= 256, summed
 * N >= 256, alignment and row pitches).  That kernel stores exactly dA's [M, K] region and raises amax_out with the exact
 * maximum of what it stored; a caller that relies on that (engine.LinearGroupOp -> the deterministic scatter's fixed-point
 * unit) asks here, so that its belief and the library's dispatch cannot drift apart.  No GPU work, no error text. */
int mml_gemm_os_serves(const mml_gemm_dgrad_desc* desc, int32_t n);

/* ------------------------------------------------------------------------------------------------
 * K4  gate: skinny linear [Gd -> ne] (no bias) + softmax over experts + expert mix.
 * Replaces gate_dnn_final_layer + softmax + matmul([B,1,Ne],[B,Ne,H]) (model/mmoe.py:80-88,
 * model/ple.py:127-152).  A group = a list of expert outputs (each [B,H]) and up to MML_MAX_GATES gates, each
 * mixing a subset of them (MMoE: every gate sees every expert; PLE CGC: task gate t sees its S specific
 * experts + the shared ones, the shared gate sees all).
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  const float* G;   /* [B, Gd] gate-DNN output (or dnn_input when gate_dnn_hidden_units == []) */
  const float* Wg;  /* [ne, Gd] nn.Linear(bias=False) weight                                   */
  float* P;         /* [B, ne] softmax(G Wg^T)                                                 */
  float* mix;       /* [B, H]  sum_e P[:,e] * E_{expert[e]}                                    */
  /* backward only: */
  const float* dmix; /* [B, H] gradient of mix                                                 */
  float* dG;         /* [B, Gd] = (dlogits Wg) (* relu'(G) if g_relu)                          */
  float* dWg;        /* [ne, Gd] = dlogits^T G                                                 */
  int64_t ldg, ldp, ldmix, lddmix, lddg;
  int32_t Gd, ne;
  int32_t g_relu;    /* 1: G is a ReLU output, fold its derivative into dG                     */
  int32_t active;    /* backward: 0 = this gate's mix was never consumed (PLE last-level shared gate, model/ple.py:146-152) */
  int32_t expert[MML_MAX_EXPERTS]; /* indices into the group's expert list                    */
} mml_gate_desc;
typedef struct {
  const float* E[MML_MAX_EXPERTS];  /* expert outputs, each [B, H]                            */
  float* dE[MML_MAX_EXPERTS];       /* backward: gradient w.r.t. each expert's PRE-activation (relu' folded in when e_relu) */
  int64_t lde[MML_MAX_EXPERTS], ldde[MML_MAX_EXPERTS];
  int32_t n_experts, n_gates, H;
  int32_t e_relu;                   /* experts end in ReLU (always true for DNN, model/utils.py:155-156) */
  int64_t B;
  mml_gate_desc gate[MML_MAX_GATES];
  /* Optional operand-magnitude slots (see "operand magnitudes" at the GEMM family), each shared by all tensors of its
   * kind: raised with max |mix| over every gate's mixture (forward), max |dE| over every expert gradient and max |dG|
   * over every gate-input gradient (backward).  NULL = not wanted. */
  uint32_t* amax_mix;
  uint32_t* amax_dE;
  uint32_t* amax_dG;
  /* bf16-storage path (K3'): bit 0 = every gate's `mix` is a bf16 [B, H] buffer (ldmix in bf16 elements), bit 1 = every
   * dE, bit 2 = every dG -- the tensors that only GEMMs read are written as their operands (round to nearest even);
   * bit 3 = every expert output E ARRIVES as bf16 (lde in bf16 elements; written that way by the layer that produced it:
   * mml_g16_tn_desc.c_bf16) and is widened exactly; everything else the kernels read stays fp32.  Only the fast row
   * kernels honour it: other shapes return MML_ERR_UNSUPPORTED when a bit is set.  With bit 3, 4 experts x <= 2 gates,
   * 128 < H <= 256, H % 8 == 0 and gate inputs of at most 128 columns the kernels run eight row columns per lane on
   * 32-lane groups (16-byte accesses to the bf16 rows, two samples per wave and trip: round 6). */
  int32_t out_bf16;
  int32_t pad_;
} mml_gate_group;
#define MML_GATE_MIX_BF16 1
#define MML_GATE_DE_BF16 2
#define MML_GATE_DG_BF16 4
#define MML_GATE_E_BF16 8
int mml_gate_mix_fwd(const mml_gate_group* grp, mml_stream_t stream);
int64_t mml_gate_mix_bwd_workspace_bytes(const mml_gate_group* grp);
int mml_gate_mix_bwd(const mml_gate_group* grp, void* workspace, int64_t workspace_bytes, mml_stream_t stream);
/* The same in two launches, like mml_gemm_grouped_wgrad_phase: phase 1 runs the row kernel (input gradients stored, the
 * per-workgroup partial sums of dWg left in the workspace), phase 2 reduces them into dWg (phase 0 = both).  Only the
 * optimizer reads dWg, so a trainer issues phase 2 off its backward chain (beside the weight-gradient GEMMs); the
 * workspace must stay untouched between the two. */
int mml_gate_mix_bwd_phase(const mml_gate_group* grp, void* workspace, int64_t workspace_bytes, int32_t phase,
                           mml_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * K5  prediction heads + loss.
 * Replaces tower_dnn_final_layer (Linear(H->1, bias=False)), PredictionLayer (x + bias, sigmoid;
 * model/utils.py:242-248), the optional domain-mask product (model/mmoe.py:101-106) and
 * sum_t F.binary_cross_entropy(reduction='sum') (model/basemodel.py:294-296) with its backward.
 * Forward-only (predict): y == NULL.
 *
 * Head kinds (mml_head_desc.kind, mml_tower_head_desc.kind): what a head predicts and what it is trained against.
 * Low byte = output form (PredictionLayer("binary") / ("regression"), model/utils.py:242-248), second byte = the loss
 * term when labels are given (model/basemodel.py:595-603: F.binary_cross_entropy / F.mse_loss / F.l1_loss, each with
 * reduction='sum').  kind == 0 is the sigmoid head with BCE.  For logit z, mask value m, label y:
 *     p  = sigmoid(z)              (MML_HEAD_OUT_SIGMOID)      |  p = z               (MML_HEAD_OUT_IDENTITY)
 *     pm = p m  (stored in prob)
 *     dz = d(pm) m p (1 - p)                                   |  dz = d(pm) m
 *     BCE: loss = -(y log pm + (1 - y) log(1 - pm)), logs clamped at -100; d(pm) = (pm - y) / max(pm (1 - pm), 1e-12)
 *     MSE: loss = (pm - y)^2,  d(pm) = 2 (pm - y)
 *     MAE: loss = |pm - y|,    d(pm) = sign(pm - y) with sign(0) = 0
 * With y == NULL (forward only, or dprob given) only the output form matters.  Identity output with BCE under labels is
 * MML_ERR_UNSUPPORTED.  Kinds mix freely inside one group; a group of kind-0 heads runs the kernels it always ran.
 * ---------------------------------------------------------------------------------------------- */
#define MML_HEAD_OUT_SIGMOID 0
#define MML_HEAD_OUT_IDENTITY 1
#define MML_HEAD_LOSS_BCE 0
#define MML_HEAD_LOSS_MSE 1
#define MML_HEAD_LOSS_MAE 2
#define MML_HEAD_KIND(out, loss) ((int32_t)(((loss) << 8) | (out)))
#define MML_HEAD_KIND_OUT(kind) ((kind) & 0xff)
#define MML_HEAD_KIND_LOSS(kind) (((kind) >> 8) & 0xff)
typedef struct {
  const float* Hin;  /* [B, H] tower output (or the stream itself when tower_dnn_hidden_units == []) */
  const float* w;    /* [H] final-layer weight ([1,H] row, or STAR's [H,1] column: same memory)       */
  const float* w2;   /* optional second factor multiplied elementwise into w (STAR: specific * shared) or NULL */
  const float* bias; /* [1] PredictionLayer bias (out.<t>.bias)                                        */
  const float* bias2;/* optional extra bias terms summed in (STAR shared+specific final biases) or NULL; [n_bias2] */
  float* dH;         /* [B, H] backward: dlogit * w (* relu'(Hin) if h_relu)                           */
  float* dw;         /* [H] backward: sum_b dlogit * Hin  (gradient of the EFFECTIVE weight w*w2)      */
  float* dbias;      /* [1] backward: sum_b dlogit                                                     */
  int64_t ldh, lddh;
  int32_t H;
  int32_t h_relu;
  int32_t n_bias2;
  int32_t mask_col;  /* column of `mask` multiplied into the probability, or -1                        */
  /* Gated head (round 6; PepNet, reference model/pepnet.py:72-78: the last PPNet layer reads h (.) 2 sigmoid(gate)):
   * gate != NULL -> the head's input is Hin (.) gate, formed in registers (the product never goes to memory);
   * backward: dH = dlogit w gate (* relu'(Hin) if h_relu), dgate = dlogit w Hin act'(gate) with act = gate_act
   * (MML_ACT_NONE / SIGMOID / SIGMOID2, the derivative taken from the stored gate value), dw = sum_b dlogit Hin gate.
   * Served by the fast row kernel only (H % 4 == 0, H <= 256, 16-byte aligned rows; fp32 dH): anything else is
   * MML_ERR_UNSUPPORTED. */
  const float* gate; /* [B, H] or NULL                                                                 */
  float* dgate;      /* [B, H] backward (required when gate != NULL and the group trains)              */
  int64_t ldgate, lddgate;
  int32_t gate_act;
  int32_t kind;      /* MML_HEAD_KIND(output form, loss); 0 = sigmoid + BCE                              */
} mml_head_desc;
typedef struct {
  int32_t n_heads;
  int32_t dh_bf16;    /* bf16-storage path (K3'): 1 = every head's dH is a bf16 [B, H] buffer (lddh in bf16 elements); fast kernel only */
  int64_t B;
  float* prob;        /* [B, ldprob] predictions (probabilities, or raw values of identity heads), head t in column t */
  int64_t ldprob;
  const float* y;     /* [B, ldy] labels or NULL (forward only)                                        */
  int64_t ldy;
  const float* mask;  /* [B, ldmask] domain mask or NULL                                               */
  int64_t ldmask;
  float* loss;        /* [1] device scalar: sum of the heads' loss terms over samples (overwritten), or NULL */
  const float* dprob; /* [B, lddprob] upstream dL/dprob used INSTEAD of the BCE gradient when y == NULL (autograd path) */
  int64_t lddprob;
  mml_head_desc head[MML_MAX_HEADS];
  uint32_t* amax_dH;  /* optional operand-magnitude slot raised with max |dH| over all heads (training), or NULL */
  uint32_t* amax_dG;  /* the same for max |dgate| over all gated heads, or NULL                                   */
} mml_head_group;
int64_t mml_head_workspace_bytes(const mml_head_group* grp);
int mml_head_fwd(const mml_head_group* grp, mml_stream_t stream);
/* forward + loss + backward of the heads in one pass (training).  With y != NULL the loss is the sum of every head's
 * term (BCE, or what its kind names); with y == NULL and dprob != NULL the heads are differentiated against the given upstream gradient. */
int mml_head_bce_fwd_bwd(const mml_head_group* grp, void* workspace, int64_t workspace_bytes, mml_stream_t stream);
/* The same in two launches: phase 1 = the row kernel (probabilities, dH), phase 2 = the reduction of the per-workgroup
 * partial sums into dw / dbias / loss (phase 0 = both); see mml_gate_mix_bwd_phase. */
int mml_head_bce_fwd_bwd_phase(const mml_head_group* grp, void* workspace, int64_t workspace_bytes, int32_t phase,
                               mml_stream_t stream);
/* The reductions (phase 2) of several head / gate groups in ONE launch (round 5): items[i] names a group whose phase 1 has
 * run into `workspace`; the result is what the phase-2 calls give one by one (dw / dbias / loss of a head group, dWg of a
 * gate group) -- in the last bits it may differ where the merged list is long enough for another reduction kernel (the
 * order of the partial sums is fixed either way).  At most 40 result tensors per call. */
#define MML_ROWS_REDUCE_HEAD 0
#define MML_ROWS_REDUCE_GATE 1
#define MML_ROWS_REDUCE_TOWER_HEAD 2   /* group = const mml_tower_head_group* (K5') */
typedef struct {
  int32_t kind; /* MML_ROWS_REDUCE_HEAD: group = const mml_head_group*; MML_ROWS_REDUCE_GATE: const mml_gate_group* */
  int32_t pad_;
  const void* group;
  void* workspace;
  int64_t workspace_bytes;
} mml_rows_reduce_item;
int mml_rows_reduce_batch(const mml_rows_reduce_item* items, int32_t n, mml_stream_t stream);
/* The kernel of this thread's last successful K4 / K5 row-kernel launch (mml_gate_mix_fwd, mml_gate_mix_bwd[_phase],
 * mml_head_fwd, mml_head_bce_fwd_bwd[_phase]; the reductions are not reported) with its template arguments, as the launch
 * site spells it -- "gate_bwd_fast_kernel<32, 4, 2, 1, 1>", "head_kernel<false>" --, or "" before the first one. */
const char* mml_rows_last_kernel(void);
/* Which of the fast gate kernels a group of this shape will get, before any buffer exists: n_gates gates, each over all
 * n_experts experts in order, expert outputs of H columns (bf16 when e_bf16), gate inputs of gd_max columns -- assuming
 * 16-byte aligned buffers and row pitches that are multiples of 8 elements.  A bit set under the process's switches
 * (MMLREC_GATE_*): what mml_gate_mix_fwd / _bwd decide is built on the same rule (csrc/rows_route.hpp), so a caller that
 * chooses storage formats by it (model/mmoe.py, engine.GateGroupOp) cannot drift from the library.  The fast kernels alone
 * honour mml_gate_group.out_bf16.  No GPU work, no error text. */
#define MML_GATE_SHAPE_FAST_FWD 1 /* the forward runs a fast row kernel                                  */
#define MML_GATE_SHAPE_FAST_BWD 2 /* the backward does                                                   */
#define MML_GATE_SHAPE_HV_FWD 4   /* ... the forward's form with eight row columns per lane (bf16 experts) */
#define MML_GATE_SHAPE_HV_BWD 8   /* ... the backward's                                                  */
int32_t mml_gate_rows_shape(int32_t H, int32_t gd_max, int32_t n_experts, int32_t n_gates, int32_t e_bf16);

/* ------------------------------------------------------------------------------------------------
 * K5' (round 6)  the top of the network in ONE launch: last tower layer (Linear(K -> N) + ReLU) -> head (Linear(N -> 1,
 * no bias) + PredictionLayer bias + sigmoid) -> optional domain-mask product -> summed BCE -> backward of all of it down to
 * dL/d(tower input).  Replaces, for every task t, tower_dnn[t] (its last layer), tower_dnn_final_layer[t], out[t] and the
 * loss terms of model/mmoe.py:93-108, model/utils.py:146-161, :242-248, model/basemodel.py:294-296 -- i.e. one
 * mml_gemm_grouped_fwd, one mml_head_bce_fwd_bwd and one mml_gemm_grouped_dgrad launch.  The tower outputs stay in
 * registers; written: prob, dH = dL/d(tower pre-activation) (the tower's weight gradient reads it), dA = dL/d(tower input)
 * (overwritten), and the head's dw / dhbias and the loss through per-workgroup partial sums (phase 2: fixed order).
 * Arithmetic: the two-plane fp16 products of the GEMM family (the tower weight's pre-cut planes in BOTH layouts,
 * mml_gemm_planes_cut; the input's magnitude slot; dH is scaled per 32-row block by its own largest magnitude), the head
 * kernel's expressions for probability, clamped-log BCE and its derivative -- or, per task, those of its `kind` (see K5:
 * identity output, squared / absolute error; tasks of different kinds share the launch).  Training only (y required).
 * Served shapes: mml_tower_head_serves (all tasks of one (N, K) in {(64, 128), (64, 64)}, 16-byte aligned rows).
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  const float* A;               /* [M, K] tower input                                                     */
  int64_t lda;
  const uint32_t* amax_a;       /* magnitude slot of A                                                    */
  const uint32_t* w_planes_fwd; /* planes of the tower weight W [N, K], MML_PLANES_ROWS, pitch ldpf words */
  const uint32_t* w_planes_bwd; /* planes of the same W, MML_PLANES_COLS, pitch ldpb words                */
  int64_t ldpf, ldpb;
  const int32_t* kexp_fwd;      /* exponents the two images were cut with                                 */
  const int32_t* kexp_bwd;
  const float* bias1;           /* [N] tower bias or NULL                                                 */
  const float* w;               /* [N] head weight                                                        */
  const float* hbias;           /* [1] PredictionLayer bias                                               */
  const float* hbias2;          /* [n_hbias2] further bias terms summed in, or NULL                       */
  float* dH;                    /* [M, N]                                                                 */
  float* dA;                    /* [M, K]                                                                 */
  int64_t lddh, ldda;
  float* dw;                    /* [N] head weight gradient                                               */
  float* dhbias;                /* [1]                                                                    */
  uint32_t* amax_dH;            /* optional magnitude slots raised with what was stored, or NULL          */
  uint32_t* amax_dA;
  int32_t K, N, n_hbias2;
  int32_t mask_col;             /* column of `mask` multiplied into the probability, or -1                */
  int32_t head;                 /* column of prob / y this task uses                                      */
  int32_t kind;                 /* MML_HEAD_KIND(output form, loss) as in mml_head_desc; 0 = sigmoid + BCE */
} mml_tower_head_desc;
typedef struct {
  int32_t n;                    /* tasks                                                                  */
  int32_t pad_;
  int64_t M;
  float* prob;                  /* [M, ldprob]                                                            */
  int64_t ldprob;
  const float* y;               /* [M, ldy] labels                                                        */
  int64_t ldy;
  const float* mask;            /* [M, ldmask] domain mask or NULL                                        */
  int64_t ldmask;
  float* loss;                  /* [1] sum of BCE over tasks and samples (overwritten), or NULL           */
  mml_tower_head_desc t[MML_MAX_HEADS];
} mml_tower_head_group;
int mml_tower_head_serves(const mml_tower_head_group* grp);            /* 1 / 0, no error text                   */
int64_t mml_tower_head_workspace_bytes(const mml_tower_head_group* grp);
/* phase 1: the launch; 2: the reduction of the partial sums; 0: both */
int mml_tower_head_fwd_bwd(const mml_tower_head_group* grp, void* workspace, int64_t workspace_bytes, int32_t phase,
                           mml_stream_t stream);


/* ------------------------------------------------------------------------------------------------
 * K3'  bf16-STORAGE GEMM family (round 5; csrc/gemm16.hip) -- BASELINE.json configs[1] ("MMoE ... KuaiRec-shaped ...
 * bf16"): the DNN layers of model/utils.py:146-161 with activations and their gradients STORED as bf16 wherever
 * producer and consumers are GEMMs (and, round 6, the expert outputs of an MMoE whose gate kernels read bf16 rows
 * sixteen bytes per lane: mml_gate_group.out_bf16 bit 3 -- one rounding of those outputs more than operand rounding at
 * the GEMMs).  Arithmetic: one v_mfma_f32_32x32x16_bf16 per 16-k block, fp32 accumulation --
 * exactly the products of mml_gemm_set_mode(1) (operands rounded to bf16, there in registers, here when they are
 * stored), with half the activation traffic and no conversion work in the kernels: bf16 tiles go HBM -> LDS by DMA and
 * LDS -> MFMA fragments as they are (ds_read_b128; the batch-reduction of the weight gradient through the transposing
 * LDS read ds_read_b64_tr_b16).  Opt-in like mode 1, outside the 1e-4 fp32 parity contract; bf16 values are
 * uint16_t bit patterns (round to nearest even).
 *   mml_cast16_batch      bf16 copies of fp32 matrices, optionally transposed: the weights of a step, once per step
 *                         ([N, K] for the forward, [K, N] for the input gradient -- both read reduction-contiguous)
 *   mml_gather16_fwd      mml_gather_fwd writing dnn_input as bf16 (the table rows rounded on the way)
 *   mml_g16_tn            C[M, N] = epilogue(sum_s A_s[M, K_s] B_s[N, K_s]^T): forward (one source, + bias, ReLU, ReLU
 *                         sign masks like mml_gemm_fwd_desc.relu_mask) and input gradient (the sources of
 *                         mml_gemm_dgrad_desc with the TRANSPOSED bf16 weights, ReLU derivative from the sign masks);
 *                         C bf16 or fp32.  M % 128 == 0, N % 64 == 0, every K_s % 64 == 0, 16-byte aligned rows.
 *   mml_g16_wgrad         dW[N, K] (+)= dC[M, N]^T A[M, K], dbias[N] (+)= column sums of dC; dC, A bf16, dW / dbias
 *                         fp32; the batch is cut into slabs, partial tiles go to the workspace and are summed in a fixed
 *                         order (bitwise reproducible).  N % 128 == 0, K % 128 == 0, M % 64 == 0.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  const float* src;   /* fp32 [rows, cols], row pitch lds (elements) */
  uint16_t* dst;      /* bf16 [rows, cols] (transpose = 0) or [cols, rows] (transpose = 1), row pitch ldd */
  int64_t rows, lds, ldd;
  int32_t cols, transpose;
} mml_cast16_desc;
int mml_cast16_batch(const mml_cast16_desc* descs, int32_t n, mml_stream_t stream);
int mml_gather16_fwd(const float* const* tables, const int64_t* vocab, const int32_t* col, int32_t F, int32_t E,
                     const float* X, int64_t ldX, int32_t dense_col0, int32_t Nd, int64_t B, uint16_t* out, int64_t ldo,
                     int32_t* status, mml_stream_t stream);
typedef struct {
  int32_t M, N;
  int32_t n_src;      /* 1 .. MML_MAX_SRC: the reduction runs over the sources one after the other */
  int32_t act;        /* MML_ACT_NONE / MML_ACT_RELU applied to (sum + bias) -- forward */
  const uint16_t* A[MML_MAX_SRC];   /* bf16 [M, K_s] */
  const uint16_t* B[MML_MAX_SRC];   /* bf16 [N, K_s]: the weight with the reduction along its rows */
  int64_t lda[MML_MAX_SRC], ldb[MML_MAX_SRC];
  int32_t K[MML_MAX_SRC];
  const float* bias;  /* [N] or NULL */
  void* C;            /* [M, N]: bf16 (c_bf16 = 1) or fp32 */
  int64_t ldc;
  int32_t c_bf16;
  int32_t accumulate; /* fp32 C only: C += result */
  uint32_t* mask_out;       /* forward, act = RELU: bit (c & 31) of mask_out[r * ldmask + (c >> 5)] = (C[r][c] > 0), or NULL */
  const uint32_t* mask_in;  /* input gradient: the result is multiplied by that bit (ReLU derivative), or NULL */
  int64_t ldmask;
} mml_g16_tn_desc;
int mml_g16_tn(const mml_g16_tn_desc* descs, int32_t n, mml_stream_t stream);
typedef struct {
  const uint16_t* dC; /* bf16 [M, N] */
  const uint16_t* A;  /* bf16 [M, K] */
  float* dW;          /* fp32 [N, K] */
  float* dbias;       /* fp32 [N] or NULL */
  int64_t lddc, lda, lddw;
  int32_t M, N, K;
  int32_t accumulate;
} mml_g16_wgrad_desc;
int64_t mml_g16_wgrad_workspace_bytes(const mml_g16_wgrad_desc* descs, int32_t n);
/* phase 0 = both launches, 1 = the partial products, 2 = their reduction (like mml_gemm_grouped_wgrad_phase) */
int mml_g16_wgrad(const mml_g16_wgrad_desc* descs, int32_t n, void* workspace, int64_t workspace_bytes, int32_t phase,
                  mml_stream_t stream);
/* Kernel symbol of the calling thread's most recent launch of this family ("" before the first). */
const char* mml_g16_last_kernel(void);

/* ------------------------------------------------------------------------------------------------
 * K6/K7  elementwise helpers for STAR / PepNet.
 *   mul:      out = a * b                                  (STAR W_spec * W_shared, model/utils.py:215;
 *                                                           PepNet hidden * gate, model/pepnet.py:77, :140)
 *   mul_bwd:  da (+)= dout * b ; db (+)= dout * a          (either may be NULL = stop-gradient)
 *   add_n:    out = sum_i in[i]                            (bias sums, gradient fan-in)
 * ---------------------------------------------------------------------------------------------- */
int mml_ew_mul(const float* a, const float* b, float* out, int64_t n, mml_stream_t stream);
int mml_ew_mul_bwd(const float* dout, const float* a, const float* b, float* da, float* db, int32_t acc_a,
                   int32_t acc_b, int64_t n, mml_stream_t stream);
/* mul_bwd with the derivative of the activation that PRODUCED an operand folded in (act_* != MML_ACT_NONE: the operand
 * holds the activation's output and this product is its only consumer; the gradient written is then the one w.r.t. the
 * pre-activation): PepNet's h * 2*sigmoid(gate) products, model/pepnet.py:72-78 -- saves the separate act' pass */
int mml_ew_mul_bwd_act(const float* dout, const float* a, const float* b, float* da, float* db, int32_t acc_a,
                       int32_t acc_b, int64_t n, int32_t act_a, int32_t act_b, mml_stream_t stream);
int mml_ew_add_n(const float* const* in, int32_t n_in, float* out, int64_t n, mml_stream_t stream);
/* n independent items in one launch (16 per kernel-argument block): out[i] (+)= sum_k x_k[i] * (y_k ? y_k[i] : 1).
 * STAR's derived parameters -- W_spec[d] * W_shared and b_spec[d] + b_shared of every head and layer
 * (SharedSpecificLinear, model/utils.py:214-216) -- and their gradients (d W_shared = sum_d dW_eff[d] * W_spec[d], ...)
 * as one call each way instead of one launch per tensor.  `d` is a HOST array.  The whole array is validated before the
 * first launch: a malformed item (its index is in mml_last_error()) returns MML_ERR_ARG and no output of the call is
 * written. */
#define MML_SUMPROD_TERMS 8
#define MML_SUMPROD_BATCH 16
typedef struct mml_sumprod_desc {
  float* out;
  const float* x[MML_SUMPROD_TERMS];
  const float* y[MML_SUMPROD_TERMS]; /* NULL = 1 */
  int64_t n;
  int32_t n_terms;
  int32_t accumulate;
  /* act != MML_ACT_NONE: the sum is multiplied by act'(.) taken from deriv_of[i], the OUTPUT of that activation (needs
   * accumulate == 0): the gradient w.r.t. the pre-activation of a factor whose only consumer is this product --
   * PepNet's h * 2*sigmoid(gate) products of all tasks of a layer in one launch each way (model/pepnet.py:72-78) */
  const float* deriv_of;
  int32_t act;
  int32_t pad_;
  uint32_t* amax_out; /* optional operand-magnitude slot (see the GEMM family) raised with max |out|, or NULL */
} mml_sumprod_desc;
int mml_sumprod_batch(const mml_sumprod_desc* d, int32_t n, mml_stream_t stream);
/* Dropout after a DNN layer's activation (reference model/utils.py:121 `self.dropout = nn.Dropout(dropout_rate)`,
 * :159 `fc = self.dropout(fc)`; training mode only -- evaluation is the identity and launches nothing):
 *   out[r, c] (+)= x[r, c] * (keep(r, c) ? 1 / (1 - p) : 0),  r < rows, c < cols (row pitches ldx / ldo; out may be x).
 * keep() is a pure function of (seed, step, site, row0 + r, c): word (c mod 4) of Philox4x32-10 with counter
 * (row0 + r, c / 4, step, site) and key (seed low, seed high), kept iff word >= floor(p * 2^32).  row0 = the position
 * of this buffer's first row in the GLOBAL batch (rank * local batch on a data-parallel rank, else 0): N ranks on a
 * split batch draw the mask one rank draws on the whole batch.  No mask is stored: the
 * backward is the SAME call on dL/d(out) (same seed / step / site).  step_dev (device int32, read by the kernel: a
 * replayed HIP graph draws a new mask every step) overrides step when not NULL.  `site` tells the layers of a model
 * apart.  The stream of masks is this library's, not torch's generator: a reference run with the same torch seed drops
 * different elements (same distribution, same arithmetic). */
int mml_dropout(const float* x, int64_t ldx, float* out, int64_t ldo, int64_t rows, int32_t cols, int64_t row0, float p,
                uint64_t seed, uint32_t site, const int32_t* step_dev, int32_t step, int32_t accumulate,
                mml_stream_t stream);
/* strided 2-D copy / accumulate: dst[r, c] (+)= src[r, c], r < rows, c < cols (concat / split of feature blocks,
 * model/pepnet.py:72, :139) */
int mml_copy2d(const float* src, int64_t lds, float* dst, int64_t ldd, int64_t rows, int32_t cols, int32_t accumulate,
               mml_stream_t stream);
/* n independent strided 2-D copies in ONE launch (item i: dst[r, c] (+)= src[r, c], r < rows, c < cols): the engine's
 * zero-padded weight copies for layers whose reduction length is not a multiple of the GEMM k-step (K0 = 303 with the
 * 63 dense AliExpress columns, configs_msl/config_AE.json:18-23), one launch per layer group instead of one per weight.
 * `d` is a HOST array. */
typedef struct mml_copy2d_desc {
  const float* src;
  int64_t lds;
  float* dst;
  int64_t ldd;
  int64_t rows;
  int32_t cols;
  int32_t accumulate;
  /* optional operand-magnitude slot (MML_AMAX_WORDS words, mml_amax_batch's format): raised with max |x| of what this item
   * stores -- the copies that assemble a GEMM operand measure it on the way (PepNet's gate inputs, model/pepnet.py:72,
   * :139: torch.cat of a detached input and the scene embedding) instead of a pass of mml_amax_batch over the result. */
  uint32_t* amax_out;
} mml_copy2d_desc;
int mml_copy2d_batch(const mml_copy2d_desc* d, int32_t n, mml_stream_t stream);
/* Up to MML_MAX_FIELDS strided column-block copies in ONE launch: for segment s, dst[s][r*ldd[s] + c] (+)= src[s][r*lds[s] + c],
 * r < rows, c < width[s].  Packs / unpacks the per-field pieces of index, row and gradient blocks around the
 * all-to-all exchange of table-sharded runs (no reference counterpart: the reference is single-process).
 * All arrays are HOST arrays of n_seg entries holding device pointers / element strides. */
int mml_copy_cols(const float* const* src, const int64_t* lds, float* const* dst, const int64_t* ldd,
                  const int32_t* width, int32_t n_seg, int64_t rows, int32_t accumulate, mml_stream_t stream);
/* BatchNorm1d inside DNN (model/utils.py:132-134, :153-154: fc -> bn -> activation; torch defaults eps 1e-5, momentum
 * 0.1).  fwd, training != 0: batch statistics (mean / rstd are written for the backward), running statistics and
 * num_batches_tracked updated in place; training == 0: running statistics.  y = act(gamma (z - mean) rstd + beta).
 * bwd: dy is the gradient w.r.t. the BN output (activation derivative already applied by the caller);
 * dgamma / dbeta are written (or accumulated), dz = gamma rstd (dy - (sum dy + xhat sum dy xhat) / B).
 * Workspace: mml_bn_workspace_bytes(B, n) for either call. */
int64_t mml_bn_workspace_bytes(int64_t B, int32_t n);
int mml_bn_fwd(const float* z, int64_t ldz, const float* gamma, const float* beta, float* running_mean, float* running_var,
               int64_t* num_batches_tracked, float* mean, float* rstd, float* y, int64_t ldy, int64_t B, int32_t n,
               int32_t act, int32_t training, float eps, float momentum, void* workspace, int64_t workspace_bytes,
               mml_stream_t stream);
int mml_bn_bwd(const float* dy, int64_t lddy, const float* z, int64_t ldz, const float* gamma, const float* mean,
               const float* rstd, float* dz, int64_t lddz, float* dgamma, float* dbeta, int32_t accumulate, int64_t B,
               int32_t n, void* workspace, int64_t workspace_bytes, mml_stream_t stream);
/* PReLU with one learnable slope per layer (model/utils.py:25-26 `nn.PReLU()`; DNN applies fc -> bn -> activation ->
 * dropout, :153-159; STAR one activation per layer for every domain, model/star.py:29-31, :47-49).  torch's semantics:
 *     forward : y  = z > 0 ? z  : alpha * z       (one fp32 multiply; z = +-0 takes the alpha * z branch)
 *     backward: dz = z > 0 ? dy : alpha * dy,     dalpha = sum over the elements with z <= 0 of dy * z
 * The backward reads z, not y: for alpha <= 0 the sign of y does not give the sign of z.
 * ONE launch serves n independent items (`d` is a HOST array, 1 <= n <= mml_prelu_max_batch(), which is >= MML_MAX_GROUP).
 * Item: z / y [rows, cols] with row pitches ldz / ldy >= cols; columns [cols, ld) are neither read nor written.  16-byte
 * accesses when every pitch of the item is a multiple of 4 and every pointer 16-byte aligned, single elements otherwise.
 * alpha is a DEVICE pointer read by the kernel when it runs (a replayed HIP graph sees what the optimizer wrote).
 * amax_out (optional): an operand-magnitude slot (MML_AMAX_WORDS words) raised with the exact max |y| (forward) /
 * max |dz| (backward, after accumulate_dz) of what the item stores -- mml_copy2d_desc.amax_out's contract.
 * Backward: dz may be dy (each element is read before it is written); accumulate_dz != 0 adds to dz.  Items that name
 * the same dalpha are summed into it in descriptor order (STAR: one slope, every domain's activations) and must agree on
 * accumulate_dalpha (!= 0: added to the old value).  dalpha is a fixed-order reduction -- lane, wave, workgroup
 * partials in the workspace (mml_prelu_workspace_bytes(n)), one ordered final sum in double -- with no float atomics:
 * two launches on the same inputs give the same bits.
 * MML_ERR_ARG: n < 1, n > mml_prelu_max_batch(), a null pointer (amax_out excepted), rows < 0, cols < 1, ld < cols,
 * a workspace that is null or too small. */
typedef struct mml_prelu_desc {
  const float* z;
  int64_t ldz;
  float* y;
  int64_t ldy;
  int64_t rows;
  int32_t cols;
  int32_t pad_;
  const float* alpha;
  uint32_t* amax_out;
} mml_prelu_desc;
typedef struct mml_prelu_bwd_desc {
  const float* dy;
  int64_t lddy;
  const float* z;
  int64_t ldz;
  float* dz;
  int64_t lddz;
  int64_t rows;
  int32_t cols;
  int32_t pad_;
  const float* alpha;
  float* dalpha;
  int32_t accumulate_dz;
  int32_t accumulate_dalpha;
  uint32_t* amax_out;
} mml_prelu_bwd_desc;
int32_t mml_prelu_max_batch(void);
int mml_prelu_batch_fwd(const mml_prelu_desc* d, int32_t n, mml_stream_t stream);
int64_t mml_prelu_workspace_bytes(int32_t n);
int mml_prelu_batch_bwd(const mml_prelu_bwd_desc* d, int32_t n, void* workspace, int64_t workspace_bytes,
                        mml_stream_t stream);
/* PCGrad gradient surgery (model/optimizer.py:10-138) over T per-objective gradients g_0 .. g_{T-1}, each the flattened
 * gradient of ALL parameters.  Every projected gradient stays in the span of the originals, pc_i = sum_k c_ik g_k, so:
 *   mml_pcgrad_gram    : ONE pass over the banks -> the T x T Gram matrix G[k][j] = <g_k, g_j> (double, symmetric)
 *   mml_pcgrad_weights : the projection loop (:50-55) as a recursion on the coefficients, in double: for i ascending,
 *                        c_i = e_i; for j in order[i*T ..]: d = sum_k c_i[k] G[k][j]; d < 0: c_i[j] -= d / G[j][j]
 *                        (G[j][j] == 0 can only meet d == 0: no division).  w[k] = (1/T) sum_i c_ik (mean weights),
 *                        w[T + k] = sum_i c_ik (sum weights), fp32; fired[i*T + j] = 1 where a projection happened, else 0.
 *   mml_pcgrad_combine : out = sum_k w'[k] bank_k per element, fp32, acc = 0 then acc = fma(w'[k], bank_k, acc) with k
 *                        ascending; w' = the mean weights where EVERY bank of the segment is non-NULL (:58), the sum
 *                        weights otherwise (:65); a NULL bank contributes nothing.  out may be one of the banks.
 * A segment is one parameter tensor: bank[t] = objective t's gradient [rows, cols] with row pitch ld (shared by the banks
 * and out), or NULL = the objective has no gradient there (zeros).  row_marks (optional, one byte per row): rows whose
 * byte is 0 hold zeros in every bank -- they are not read, and combine does not write them.  `s` is a HOST array of any
 * length n >= 1.  16-byte accesses where ld % 4 == 0 and every pointer of the segment is 16-byte aligned, single elements
 * otherwise.  gram takes the fp32 products in double (exact) and adds them in a fixed order -- lane, wave, workgroup
 * partials in the workspace (mml_pcgrad_workspace_bytes), one ordered final sum -- with no float atomics: two launches on
 * the same inputs give the same bits.  `order` ([T*T] int32, row i = the order in which g_i meets the g_j), gram, w
 * and fired are DEVICE pointers.
 * MML_ERR_ARG: T < 1, T > MML_PCGRAD_MAX_TASKS, n < 1, a null array, rows < 0, cols < 1, ld < cols, a segment whose banks
 * are all NULL, a null out (combine), a workspace that is null or too small.  (The entries of `order` are device data
 * and are not checked: an entry outside [0, T) is skipped by the kernel.) */
#define MML_PCGRAD_MAX_TASKS 8
typedef struct mml_pcgrad_seg {
  const float* bank[MML_PCGRAD_MAX_TASKS];
  float* out;
  int64_t rows;
  int64_t ld;
  int32_t cols;
  int32_t pad_;
  const uint8_t* row_marks;
} mml_pcgrad_seg;
int64_t mml_pcgrad_workspace_bytes(const mml_pcgrad_seg* s, int32_t n, int32_t T);
int mml_pcgrad_gram(const mml_pcgrad_seg* s, int32_t n, int32_t T, double* gram, void* workspace,
                    int64_t workspace_bytes, mml_stream_t stream);
int mml_pcgrad_weights(const double* gram, const int32_t* order, int32_t T, float* w, int32_t* fired,
                       mml_stream_t stream);
int mml_pcgrad_combine(const mml_pcgrad_seg* s, int32_t n, int32_t T, const float* w, mml_stream_t stream);
/* One objective's gradient leaves the buffers the backward writes: out = bank[0] over the rows of every segment (the
 * marked rows where row_marks is given; the other banks are ignored), and with clear != 0 those rows of bank[0] are
 * zeroed behind the copy -- the table accumulators the scatter adds into start the next objective's pass at zero.
 * MML_ERR_ARG as for mml_pcgrad_combine with T = 1, and for out == bank[0]. */
int mml_pcgrad_stash(const mml_pcgrad_seg* s, int32_t n, int32_t clear, mml_stream_t stream);
/* DomainBatchNorm (model/utils.py:553-636; STAR applies it after its first star layer when forward() is given a domain
 * mask, model/star.py:50-51).  gamma / beta are unregistered there, frozen at (1, 0).  Training mode normalises with
 * the statistics of the WHOLE batch for every domain (= mml_bn_fwd with gamma 1 / beta 0; the caller issues that) and
 * mml_domain_bn_update moves the per-domain population statistics:
 *     pop_mean[d] = decay pop_mean[d] + (1 - decay) mean(x[argmax(mask) == d]),  pop_var[d] with the unbiased variance
 * for EVERY domain, like the reference (a domain without samples gets NaN, one with a single sample a NaN variance).
 * Eval mode: y[b] = sum_d mask[b, d] (x[b] - pop_mean[d]) / sqrt(pop_var[d] + eps)  (mml_domain_bn_eval).
 * pop_mean / pop_var are [D, n] device arrays. */
int mml_domain_bn_update(const float* x, int64_t ldx, const float* mask, int64_t ldm, int64_t B, int32_t n, int32_t D,
                         float* pop_mean, float* pop_var, float decay, mml_stream_t stream);
int mml_domain_bn_eval(const float* x, int64_t ldx, const float* mask, int64_t ldm, const float* pop_mean,
                       const float* pop_var, float* y, int64_t ldy, int64_t B, int32_t n, int32_t D, float eps,
                       mml_stream_t stream);
/* SNR-trans routing weights (model/snr_trans.py:38-50).  n_blocks = outputs x inputs blocks of `block` floats each:
 * fwd  W[b] = z(u[b], alpha) * M[b]  with the hard-concrete z = clamp(sigmoid(log u - log(1-u) + log(alpha)/beta)
 *      * (eps - gamma) + gamma, 0, 1);  the routing is then one [K,N] GEMM per output on the concatenated inputs;
 * bwd  dz[b] = <dW[b], M[b]>, du[b] (+)= dz[b] dz/du, dalpha (+)= sum_b dz[b] dz/dalpha (fixed order).
 * M is the reference's unregistered (hence frozen) trans_matrix stack.
 * zw = 1: one coefficient per block (u has n_blocks entries); zw = units: one per output column of a block (MSSM,
 * model/mssm.py:26-29: u has n_blocks * zw entries and is itself unregistered there -> du may be null). */
int mml_snr_gate_weights_fwd(const float* u, const float* alpha, const float* M, float* W, int32_t n_blocks,
                             int64_t block, int32_t zw, float beta, float gamma, float eps, mml_stream_t stream);
int mml_snr_gate_weights_bwd(const float* dW, const float* M, const float* u, const float* alpha, float* du,
                             float* dalpha, int32_t acc_u, int32_t acc_alpha, int32_t n_blocks, int64_t block,
                             int32_t zw, float beta, float gamma, float eps, float* workspace /* n_blocks floats */,
                             mml_stream_t stream);
/* Two-token attention of AITM (model/aitm.py:84-93): per sample, tokens t = 0, 1 with V_t, K_t, Q_t in R^H:
 * s_t = <K_t, Q_t> / sqrt_h, a = softmax(s_0, s_1), out = a_0 V_0 + a_1 V_1.  fwd writes out and (if non-null) the
 * weights A [B,2]; bwd reads A and dout and OVERWRITES dV, dK, dQ of both tokens.  All pointers are device pointers,
 * leading dimensions in elements. */
typedef struct mml_attn2_desc {
  const float* V[2];
  const float* K[2];
  const float* Q[2];
  int64_t ldv[2], ldk[2], ldq[2];
  float* out;
  int64_t ldo;
  float* A;
  const float* dout;
  int64_t lddo;
  float* dV[2];
  float* dK[2];
  float* dQ[2];
  int64_t lddv[2], lddk[2], lddq[2];
  int64_t B;
  int32_t H;
  float sqrt_h; /* the divisor: (float)sqrt(H) in the reference */
} mml_attn2_desc;
int mml_attn2_fwd(const mml_attn2_desc* d, mml_stream_t stream);
int mml_attn2_bwd(const mml_attn2_desc* d, mml_stream_t stream);
/* ESMM output stage (model/esmm.py:58-62): p_out[b] = (ctr, ctr * cvr) from the two head probabilities p_raw[b] = (ctr,
 * cvr).  With labels y: loss[0] = summed BCE of both outputs (model/basemodel.py:294-296) and d_raw = dLoss / d(ctr, cvr);
 * without labels but with d_out (= dL / d p_out from autograd): d_raw by the chain rule.  Feed d_raw to
 * mml_head_bce_fwd_bwd as `dprob`.  Any of y, d_out, d_raw, loss may be null. */
int mml_esmm_combine(const float* p_raw, int64_t ldr, const float* y, int64_t ldy, const float* d_out, int64_t lddo,
                     float* p_out, int64_t ldo, float* d_raw, int64_t lddr, float* loss, int64_t B, mml_stream_t stream);
/* APG (model/apg.py:9-118, the use_uv_shared / no-mf_p branch main.py builds).  The per-sample generated [k,k] weight
 * W_b = reshape(Linear_kk(scene_b)) and bias c_b = Linear_bias(scene_b) applied to the low-rank activation o1_b
 * (apg.py:77-80, :100-104) are ONE ordinary GEMM  o2 = z W_cat + bb  on
 *     z_b = [ o1_b (x) s_b  (k*E, index i*E+e) | o1_b (k) | s_b (E) | zeros up to Kf ]
 * against W_cat [Kf, k] ([K,N] layout): rows i*E+e = Wkk[(i*k+j), e], rows k*E+i = bkk[i*k+j], rows k*E+k+e = Wb[j, e].
 *   mml_apg_features_fwd  writes z;  mml_apg_features_bwd  do1 (+)= dz contracted with s (the scene embedding is
 *   detached in the reference: no gradient to s);  mml_apg_weights  dir 0: packs W_cat from (Wkk [k*k,E], bkk [k*k],
 *   Wb [k,E]); dir 1: unpacks dW_cat into their gradients (accumulating where acc_* != 0). */
int mml_apg_features_fwd(const float* o1, int64_t ldo1, const float* s, int64_t lds, float* z, int64_t ldz, int64_t B,
                         int32_t k, int32_t E, int32_t Kf, mml_stream_t stream);
int mml_apg_features_bwd(const float* dz, int64_t lddz, const float* s, int64_t lds, float* do1, int64_t lddo1,
                         int64_t B, int32_t k, int32_t E, int32_t accumulate, mml_stream_t stream);
int mml_apg_weights(float* Wkk, float* bkk, float* Wb, float* Wcat, int64_t ldw, int32_t k, int32_t E, int32_t dir,
                    int32_t acc_kk, int32_t acc_bkk, int32_t acc_wb, mml_stream_t stream);
/* ESCM output stage and loss (model/escm.py:74-112 and the loss branch of BaseModel.fit, model/basemodel.py:284-292):
 * p_out[b] = (ctr, cvr, ctr * cvr) from the two head probabilities p_raw[b] = (ctr, cvr).  With labels y [B,2]:
 *   loss = BCE_sum(ctr, y0) + cf_w * L1 * S + global_w * BCE_sum(ctr * cvr, y1),   L1 = BCE_sum(cvr, y1),
 *   S = sum_b y0_b * clip(1 / max(ctr_b * N, 1e-6), -15, 15),  N = sum_b y0_b      (counterfact_ipw, escm.py:98-112,
 *   the mean over the batch cancels the factor batch_size; the gradient flows through the inverse propensity, as it
 *   does in the reference), and d_raw = dLoss / d(ctr, cvr).  Without labels but with d_out (= dL / d p_out [B,3] from
 *   autograd): d_raw by the chain rule.  Feed d_raw to mml_head_bce_fwd_bwd as `dprob`. */
int mml_escm_combine(const float* p_raw, int64_t ldr, const float* y, int64_t ldy, const float* d_out, int64_t lddo,
                     float* p_out, int64_t ldo, float* d_raw, int64_t lddr, float* loss, int64_t B, float cf_w,
                     float global_w, mml_stream_t stream);
/* ----------------------------------------------------------------------------------------------
 * Per-batch AUC on the device.  Replaces sklearn.metrics.roc_auc_score run on the host for every
 * training step (model/basemodel.py:316-331; the epoch log averages the per-step values, :335-337): for every segment
 * of `seg` consecutive rows (the last one may be shorter) and every column c < cols,
 *     auc[s * cols + c] = roc_auc_score(y[rows, c] > 0.5, pred[rows, c])
 * with sklearn's tie handling (Mann-Whitney with half credit inside a tie group, evaluated in integer arithmetic), NaN
 * when the segment holds a single class (sklearn raises ValueError there).  seg <= 4096 (one workgroup sorts one
 * segment column in LDS); larger segments return MML_ERR_UNSUPPORTED.  `auc` is a DEVICE array of ceil(n/seg)*cols doubles.
 * ---------------------------------------------------------------------------------------------- */
int mml_auc_segments(const float* pred, int64_t ldp, const float* y, int64_t ldy, int64_t n, int32_t cols, int32_t seg,
                     double* auc, mml_stream_t stream);
/* The same AUC for segments of ANY length, with optional row masks: a multi-workgroup radix sort of the scores
 * (csrc/auc_sort.hip).  Whole-set metrics (BaseModel.evaluate, the masked per-domain columns of the CLI's result row,
 * reference main.py:136-144) and the per-batch train AUC of batches above 4096 rows use it.
 *   problems   `seg` consecutive rows (seg == 0 or seg >= n: one segment of n rows; the last segment may be short) times
 *              a column c < cols is one independent problem s * cols + c.  n * cols < 2^31 keys per call.
 *   labels     a row is positive iff y[r * ldy + c] > 0.5 (as in mml_auc_segments).
 *   mask       NULL: every row counts.  Otherwise row r takes part in column c iff
 *              mask[r * ldm + (mask_cols == 1 ? 0 : c)] != 0  (masked_select before scoring); mask_cols is 1 or cols.
 *   result     auc[s * cols + c] = (double)2U / (2.0 * P * N), NaN when P == 0 or N == 0, with
 *              counts[3 * (s * cols + c) + {0, 1, 2}] = {2U, P, N} (counts may be NULL) and
 *              2U = sum over positives of (2 * #negatives with a smaller score + #negatives with an equal score):
 *              sklearn's roc_auc_score in integer arithmetic.  2U <= 2 * P * N <= n^2 / 2 < 2^61 for every n the call
 *              accepts, so the 64-bit sums cannot overflow.  +0.0 and -0.0 are one tie group; every finite fp32 score
 *              is accepted, negative ones included.  A NaN or infinite score at a PARTICIPATING row sets bit 4 (value 16)
 *              of *status (a device int32 the caller cleared) and makes that problem's auc NaN.
 *   rules      nothing is allocated or synchronised; HIP-graph capturable; every sum is an integer sum, so the result is
 *              bitwise repeatable and independent of the order of the rows inside a segment.  `workspace` is a device
 *              buffer of at least mml_auc_sorted_workspace_bytes(n, cols, seg) bytes (8-byte aligned; -1 for extents the
 *              call refuses); a shorter one is MML_ERR_ARG, as are mask_cols outside {1, cols} and n * cols >= 2^31.
 *              n == 0 is MML_OK.  mml_auc_sorted_tile(): keys of one scatter tile (the unit a workgroup ranks in LDS). */
int32_t mml_auc_sorted_tile(void);
int64_t mml_auc_sorted_workspace_bytes(int64_t n, int32_t cols, int64_t seg);
int mml_auc_sorted(const float* pred, int64_t ldp, const float* y, int64_t ldy, const float* mask, int64_t ldm,
                   int32_t mask_cols, int64_t n, int32_t cols, int64_t seg, void* workspace, int64_t workspace_bytes,
                   double* auc, int64_t* counts, int32_t* status, mml_stream_t stream);
/* dst = act'(y) * dy for MML_ACT_SIGMOID2 / SIGMOID / RELU given the forward OUTPUT y (GateNN backward) */
int mml_act_bwd(const float* y, const float* dy, float* dst, int64_t n, int32_t act, mml_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * K8  optimizers (torch.optim.{SGD,Adam,Adagrad,RMSprop} defaults; model/basemodel.py:313, :569-584).
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  float* param; const float* grad; /* [n] */
  float* state1;                   /* Adam m | Adagrad sum | RMSprop square_avg | SGD unused (NULL) */
  float* state2;                   /* Adam v | others NULL                                          */
  int64_t n;
  /* regulariser of this tensor (BaseModel.get_regularization_loss, model/basemodel.py:524-540: total_loss +=
   * sum(l1 |p|) + sum(l2 p^2)): the update sees grad + l1 * sign(p) + 2 * l2 * p.  0 = none. */
  float l1, l2;
  /* Split dense table update (the reference's dense optimizer, model/basemodel.py:313, with its 2.7 GB table stream
   * taken off the critical path): when skip_rows != NULL the tensor is a [rows, row_elems] table and every row whose
   * bit is set in skip_rows (the `seen` bitmap mml_index_unique builds from the batch's indices BEFORE the forward)
   * is left untouched -- those rows get their update, with their gradient, from mml_opt_step_rows after the scatter.
   * All other rows have a zero gradient this step; with zero_grads != 0 the kernel does not even read `grad` for them
   * (the accumulators are all-zero between steps).  Together the two launches are exactly one dense step. */
  const uint32_t* skip_rows;
  int32_t row_elems;
  int32_t zero_grads;
  /* Marked gradients (single-launch dense table update): grad_marks != NULL makes the tensor a [rows, row_elems] table
   * with one byte per row; a row whose byte is 0 has an all-zero gradient (the accumulators are all-zero between steps
   * and mml_scatter_bwd marks every row it adds to, see its row_marks) and `grad` is not read for it -- 4 of the 28
   * bytes per parameter of a dense Adam step, for 99 % of the rows.  The kernel clears the bytes it finds set.
   * Needs row_elems % 4 == 0 with row_elems / 4 a power of two <= 64, 16-byte aligned tensors, no skip_rows. */
  uint8_t* grad_marks;
  /* Deferred totals of the deterministic scatter (mml_scatter_bwd_det with MML_SCATTER_DET_DEFER_TOTALS): acc64 != NULL
   * makes the gradient of a MARKED row grad + from_fixed(acc64 row) -- every non-zero 64-bit total converted with the
   * exponent of the slot acc_amax (MML_AMAX_WORDS words) and acc_shift = mml_scatter_det_shift(B), exactly what the
   * scatter's second launch would have added to `grad` -- and the kernel zeroes the totals it used.  Unmarked rows read
   * neither buffer.  Needs grad_marks, a 16-byte aligned [rows, row_elems] int64 array and the streaming launch; a
   * launch that holds such a tensor takes grad_marks on every tensor.  All zero: the tensor is as before. */
  int64_t* acc64;
  const uint32_t* acc_amax;
  int32_t acc_shift;
  int32_t acc_pad_;
  /* Warm rows (Adam / RMSprop / Adagrad tables whose moments start at zero): warm_rows != NULL is one byte per table row,
   * 0 = "state1 / state2 of this row are still all zero".  Such a row with an unmarked (zero) gradient is left exactly
   * where it is by the update (m' = v' = 0, p' = p - step * 0), so the kernel neither reads nor writes it; a marked row
   * gets its byte set (plain byte store, by the lane that clears the mark), warm unmarked rows are updated as ever.  The
   * caller owns the map: all zero when the moments are created as zeros, and set to 1 for every row a writer of
   * state1 / state2 other than this launch may have touched.  Same needs as grad_marks and honoured only together with
   * it (the streaming launch); the tensor must carry no regulariser (l1 = l2 = 0).  NULL: every row is updated. */
  uint8_t* warm_rows;
} mml_opt_tensor;
typedef struct {
  int32_t kind;      /* MML_OPT_* */
  int32_t step;      /* 1-based step number used for Adam bias correction when step_dev == NULL */
  const int32_t* step_dev; /* optional device counter (hipGraph replay): the kernel reads *step_dev instead */
  float lr, beta1, beta2, eps, alpha;
  int32_t zero_grad; /* 1: write zeros over grad after use (keeps dense table-gradient accumulators clean) */
  /* > 0: cap on the workgroups of a dense launch.  A streaming launch normally fills every wave slot of the chip (8
   * workgroups per CU); the early half of the split table update runs BESIDE the forward / backward kernels and must
   * leave them slots (uncapped, a B = 4 096 step's GEMMs waited 0.3 ms for a slot), and it has the whole forward +
   * backward to finish in. */
  int32_t max_blocks;
  /* Loop of the marked streaming launch over tensors with a warm map.  0: a lane reads one aligned dword of marks and one
   * of warm bytes (four rows), the wave compacts its live rows and shares their chunks out among its lanes.  1: the loop
   * before that (a byte of each map per 16-byte chunk), kept for A/B runs; a tensor whose maps are not 4-byte aligned takes
   * it either way.  The same bits in both.  (The field fills what was the struct's tail padding: its size is unchanged.)
   * Where loop 0 runs: a launch ALL of whose tensors carry a warm map with 4-byte aligned map pointers runs on one grid
   * sized for the chip (8 workgroups per compute unit, no more than the launch would get otherwise, max_blocks included),
   * the 256-row spans of all tensors dealt to its waves; any other launch on the workgroups of each tensor.
   * 2: loop 0 on the per-tensor workgroups in every launch (A/B arm).  3: as 0 with 4 workgroups per compute unit, which
   * is what fits the chip at once (A/B arm). */
  int32_t cold_loop;
} mml_opt_hyper;
/* The constants of one optimizer step, computed once per step on the device by mml_opt_step_begin instead of by every
 * workgroup of every optimizer launch: Adam's lr / (1 - beta1^step) and 1 / sqrt(1 - beta2^step) (the double-precision
 * expressions of torch.optim.Adam, the same bits as the kernels' own), and the step they belong to.  16 bytes on the
 * device, 16-byte aligned. */
typedef struct {
  int32_t step;
  float step_size;
  float inv_bc2s;
  int32_t pad_;
} mml_opt_step_consts;
/* Start of a step, ONE single-thread launch: *step_dev += delta, then *consts = the constants of the new step under
 * hyper's kind / lr / beta1 / beta2 (hyper->step and hyper->step_dev are not read).  The library remembers that `consts`
 * belongs to `step_dev` under those four values: mml_opt_step_dense and mml_opt_step_rows launched afterwards with
 * hyper->step_dev == step_dev and the same four values have their kernels read *consts instead of computing the
 * constants per workgroup -- at run time, so a captured [begin, update] sequence replays correctly.  A kernel that finds
 * consts->step != *step_dev (somebody else moved the counter) computes them itself.  `consts` must stay allocated as
 * long as the binding exists: until mml_opt_step_unbind(step_dev), a mml_counter_update on step_dev, or another
 * mml_opt_step_begin on it.  Other hyper values, a host step (step_dev == NULL) or no binding: as before. */
int mml_opt_step_begin(int32_t* step_dev, int32_t delta, const mml_opt_hyper* hyper, mml_opt_step_consts* consts,
                       mml_stream_t stream);
int mml_opt_step_unbind(const int32_t* step_dev);
/* dense update of up to MML_MAX_OPT_TENSORS whole tensors in one launch (tables included: the reference's
 * optimizer touches every row of every table every step) */
int mml_opt_step_dense(const mml_opt_tensor* tensors, int32_t n, const mml_opt_hyper* hyper, mml_stream_t stream);
/* sparse-row update: only rows listed in touched[0 .. *touched_count) (global row ids over the concatenated
 * tables; table f owns [rowbase[f], rowbase[f+1])).  Exactly equal to the dense update for SGD and Adagrad
 * (rows with zero gradient do not move); for Adam/RMSprop it is the "lazy" variant, NOT the reference's result.
 * Re-zeroes the gradient rows and clears their `seen` bits. */
int mml_opt_step_rows(float* const* tables, float* const* grad_tables, float* const* state1, float* const* state2,
                      uint32_t* const* seen, const int64_t* rowbase, int32_t F, int32_t E,
                      const int32_t* touched, const int32_t* touched_count, int32_t touched_cap,
                      int32_t* const* last /* per-table [V] "row is current as of step" words, or NULL */,
                      const mml_opt_hyper* hyper, mml_stream_t stream);
/* Lazy-EXACT dense Adam/RMSprop for the tables.  The reference's optimizer updates every row every step: a row with
 * zero gradient still decays its moments and moves by lr_t * m_t / (sqrt(v_t / bc2_t) + eps).  Those zero-gradient
 * steps are a deterministic function of (p, m, v, step range), so they can be replayed when a row is next READ:
 *   mml_opt_catchup_rows  replays steps last[row]+1 .. target for the listed rows (target = *step_dev - 1 or
 *                         hyper->step - 1: the state the reference has before the current step), with the same
 *                         per-step arithmetic as mml_opt_step_dense and an early exit once the update falls below
 *                         half an ulp of p (from then on only the moments decay, in closed form);
 *   mml_opt_catchup_dense does the same for EVERY row of one table (before evaluation / checkpointing).
 * Together with mml_opt_step_rows(..., last, ...) this reproduces the dense trajectory while touching only the rows
 * of the current batch.
 * Any E in [1, 64]: a row's elements are adjacent lanes of one wave (a group of the next power of two at or above E,
 * the surplus lanes idle), all of which read last[row] before the row's first lane publishes the new step.  E > 64 is
 * refused with MML_ERR_ARG by both entry points (a row would not fit one wave).  A row listed twice is undefined. */
int mml_opt_catchup_rows(float* const* tables, float* const* state1, float* const* state2, int32_t* const* last,
                         const int64_t* rowbase, int32_t F, int32_t E, const int32_t* touched,
                         const int32_t* touched_count, int32_t touched_cap, const mml_opt_hyper* hyper,
                         mml_stream_t stream);
int mml_opt_catchup_dense(float* table, float* state1, float* state2, int32_t* last, int64_t V, int32_t E,
                          const mml_opt_hyper* hyper, mml_stream_t stream);
/* *counter += delta (single thread): Adam step counter, touched-list reset (delta = -*counter when reset != 0) */
int mml_counter_update(int32_t* counter, int32_t delta, int32_t reset, mml_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MMLREC_H */
