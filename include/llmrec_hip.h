/* llmrec_hip.h - C ABI of the MI355X (gfx950) hot path of LLMRec Stage 2.
 *
 * The reference (HKUDS/LLMRec) has no plugin / FFI layer: every FLOP on its hot path is an ATen
 * call made from Python. Each entry point below replaces one group of those call
 * sites; the reference file:line it stands in for is cited on the declaration. The Python host
 * (llmrec_amd/ops.py) binds these with ctypes and passes raw device pointers
 * (tensor.data_ptr()) plus the hipStream_t of torch's current stream; INTEGRATION.md shows the
 * stub a maintainer of the reference would add.
 *
 * Conventions
 *   - every function returns int: 0 = LLMREC_OK, negative = error (llmrec_status_string());
 *     llmrec_last_error() gives the thread-local detail message. Nothing throws.
 *   - all pointers are DEVICE pointers unless the name ends in _host; matrices are row-major fp32
 *     with an explicit leading dimension in ELEMENTS (ld >= number of columns).
 *   - no entry point allocates, frees or synchronises: scratch comes from the caller
 *     (sizes from the matching *_workspace_bytes query), so every call is hipGraph-capturable.
 *     The two exceptions are the one-time set-up routines llmrec_csr_build and
 *     llmrec_spmm_plan_count, which synchronise the stream to return a count to the host.
 *   - indices: COO input int64 (torch's sparse layout, reference main.py:131); CSR row pointers
 *     and column indices int32 (nnz < 2^31 in every BASELINE.json config); byte/element offsets
 *     into X/Y are computed in 64 bit inside the kernels (50 M rows x 128 floats > 2^31).
 */
#ifndef LLMREC_HIP_H
#define LLMREC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LLMREC_ABI_VERSION 8

enum {
    LLMREC_OK = 0,
    LLMREC_EINVAL = -1,        /* bad argument (null pointer, negative size, misaligned ld ...) */
    LLMREC_EHIP = -2,          /* a HIP runtime call or kernel launch failed */
    LLMREC_EWORKSPACE = -3,    /* caller workspace smaller than the *_workspace_bytes answer */
    LLMREC_EUNSUPPORTED = -4   /* shape outside the compiled kernel family */
};

typedef void* llmrec_stream_t; /* hipStream_t */

int llmrec_abi_version(void);
const char* llmrec_status_string(int status);
const char* llmrec_last_error(void);

/* ------------------------------------------------------------------------------------------
 * R1  graph ingest: COO -> CSR.          replaces scipy csr_norm + matrix_to_tensor and the
 *                                        COO->CSR conversion torch.sparse.mm does per call
 *                                        (reference main.py:84-93,114-134)
 * Sorts (row, col) pairs (radix sort, 64-bit keys) so each CSR row has ascending columns;
 * duplicate (row, col) entries are kept (torch.sparse.mm sums them too). val may be NULL
 * (pattern-only). Passing (col, row) builds the CSR of the transpose.
 * ------------------------------------------------------------------------------------------ */
int64_t llmrec_csr_build_workspace_bytes(int64_t n_rows, int64_t nnz);
int llmrec_csr_build(int64_t n_rows, int64_t n_cols, int64_t nnz,
                     const int64_t* coo_row, const int64_t* coo_col, const float* coo_val,
                     int32_t* rowptr /* n_rows+1 */, int32_t* colidx /* nnz */, float* val /* nnz or NULL */,
                     void* workspace, int64_t workspace_bytes, llmrec_stream_t stream);

/* scale[r] = fp32((deg_r + 1e-8)^-1/2), 0 for empty rows     (reference main.py:115-117) */
int llmrec_degree_scale(int64_t n_rows, const int32_t* rowptr, float* scale, llmrec_stream_t stream);

/* flag_out[0] = 1 if every row's values are one constant (then row_const[r] = that constant,
 * 0 for empty rows) else 0. Lets the SpMM drop the 4 B/nnz value stream: the reference's
 * normalised adjacency is diag(s) * R with binary R (reference main.py:123-126). */
int llmrec_csr_row_constant(int64_t n_rows, const int32_t* rowptr, const float* val,
                            float* row_const, int32_t* flag_out, llmrec_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * R2  SpMM  Y = diag(row_scale) * (P (.) val) * diag(col_scale) * X
 *                                        replaces torch.sparse.mm / torch.mm(sparse, dense)
 *                                        (reference Models.py:57-61 and its 20 call sites
 *                                        :153-157,162-163,166-167,176-180) and, with col_scale,
 *                                        the transposed SpMM autograd runs for dX = A^T dY.
 * val, row_scale, col_scale may each be NULL (= all ones). d = columns of X and Y.
 * Rounding of the col_scale form: the kernel accumulates fma(col_scale[c], X[c], acc). The Python host (llmrec_amd/ops.py::spmm_raw) runs
 * pattern-only operands of HBM-bound graphs (nnz >= 4 M) as A (c . X) instead - X pre-scaled by one dense pass into a cached scratch, then
 * this call with col_scale = NULL: acc += round(c x), one rounding more per term (<= 1 ulp of each product; the sums agree to fp32 round-off,
 * not bit for bit, with the fma form used below that size).
 * Rows are bucketed by length (the plan calls below; thresholds chosen by the host) and all buckets run in ONE launch:
 *   nnz <= LLMREC_SPMM_LONG_ROW   one lane group (d/4 lanes) per row,
 *   nnz <= t_wave                 one wavefront per row                  (list wave_rows),
 *   nnz <= t_block                one 512-thread block per row           (list block_rows),
 *   longer                        pieces of `segment` nnz, one block each, partial sums in `partials` (caller scratch,
 *                                 plan.n_segments * d floats) added in a fixed order by a second launch
 *                                 (lists split_rows / split_seg_begin / seg_split).
 * Every summation tree is fixed by (nnz, thresholds, d): results are run-to-run deterministic, no float atomics.
 * llmrec_amd/ops.py picks 32 nnz per lane group for launch-bound (L2-resident) graphs, 128 for HBM-bound ones.
 * slice_width > 0 (must divide d; epilogue op NONE only): the operand is processed as d / slice_width independent
 * column slices - (row, slice) tasks - which gives a launch-bound graph the parallelism and latency of a narrow product.
 * Epilogue on the finished row r (t = alpha * Z[r] + result[r], Z may be NULL or alias Y):
 *   LLMREC_SPMM_EPI_NONE          Y[r] = t                       (Z = Y, alpha = 1: "Y += A X")
 *   LLMREC_SPMM_EPI_SOFTMAX       Y[r] = softmax(t) over the d columns           (reference Models.py:176-177)
 *   LLMREC_SPMM_EPI_SOFTMAX_BWD   Y[r] = S[r] * (t - sum(t * S[r]))              (its backward; S = the forward output)
 * and finally an optional per-row scale of the OUTPUT (epilogue.post_scale).
 * ------------------------------------------------------------------------------------------ */
#define LLMREC_SPMM_LONG_ROW 32    /* rows with more nnz leave the lane-group bucket */

typedef struct {
    int32_t t_wave, t_block, segment;                      /* LONG_ROW <= t_wave <= t_block, segment >= LONG_ROW */
    int32_t n_wave_rows;  const int32_t* wave_rows;        /* rows with LONG_ROW < nnz <= t_wave */
    int32_t n_block_rows; const int32_t* block_rows;       /* rows with t_wave < nnz <= t_block */
    int32_t n_split_rows; const int32_t* split_rows;       /* rows with nnz > t_block */
    const int32_t* split_seg_begin;                        /* [n_split_rows] first piece of each split row */
    int32_t n_segments;   const int32_t* seg_split;        /* [n_segments] index into split_rows */
    /* Round 6 - PERMUTED CSR (pattern-only operands). slot_row != NULL: the rowptr / colidx arguments of llmrec_spmm_f32 are a copy of the operand's
     * CSR whose rows are stored in the order they are visited (llmrec_csr_permute_rows): slots [0, n_short_rows) = the lane-group bucket (nnz <=
     * LONG_ROW, empty rows included), then the wavefront, block and split rows; CSR row `slot` is output row slot_row[slot] (Y, Z, S, row_scale,
     * post_scale and the row flags are addressed by OUTPUT row) and the four lists hold slots. llmrec_amd/ops.py orders every bucket by descending
     * length class (power-of-two bucket of nnz), ascending row id within a class: a wavefront's 64 / LPR rows then have (almost) equal lengths
     * and finish together, and the index stream stays sequential - profiles/experiments/r06_spmm_order.md. Results do not depend on the order. */
    int32_t n_short_rows; const int32_t* slot_row;
} llmrec_spmm_plan_t;

#define LLMREC_SPMM_EPI_NONE 0
#define LLMREC_SPMM_EPI_SOFTMAX 1
#define LLMREC_SPMM_EPI_SOFTMAX_BWD 2
typedef struct {
    int32_t op; float alpha;
    const float* Z; int64_t ldz;
    const float* S; int64_t lds;
    const float* post_scale;     /* [n_rows] or NULL: Y[r] = post_scale[r] * op(t) - lets the CONSUMER of Y run without a per-edge
                                    col_scale gather (dX = R diag(s) g is computed as R (s . g)) */
    /* Operand sparsity (the backward of the last propagation layer: the gradient that enters it is non-zero only in the rows of the
     * batch's items, its product only in the rows of their neighbours - reference Models.py:176-186 differentiated):
     *   x_row_mask [n_cols] or NULL: rows of X whose byte differs from x_mask_active (1..255) are PROMISED all-zero and are not read
     *                 (they may hold anything); the result equals the unmasked product on the promised zeros up to the sign of a zero;
     *   y_row_flag [n_rows] or NULL: written for every row: x_mask_active if the row's result can be non-zero - an active X row was
     *                 gathered, or z_row_flag[row] == x_mask_active (a non-zero row of Z); rows of the long-row buckets are always
     *                 flagged - else 0: the mask for the next product in the chain (row-local epilogues map zero rows to zero rows);
     *   z_row_flag [n_rows] or NULL (may alias y_row_flag);
     *   y_row_gate [n_rows] or NULL: rows whose byte differs from x_mask_active are PROMISED to have no active neighbour and a zero Z row:
     *                 they are written as zeros before the index list of the row is even read (llmrec_mark_neighbours_u8 computes such a gate
     *                 from the list of active columns - a sweep over THEIR adjacency instead of the one of every row);
     *   y_row_needed [n_rows] or NULL: output rows whose byte differs from x_mask_active are NOT COMPUTED AND NOT WRITTEN (their previous
     *                 contents stay) - for a product whose consumers read only marked rows (the last propagation layer of a training step:
     *                 the loss reads the rows of the batch, the next product the rows those reach). Needs x_mask_active, not x_row_mask;
     *                 rows of the long-row buckets are always computed.
     *   rows_listed_only != 0: ONLY the rows in the lists of the plan (wavefront / block / split rows) are computed - with a plan built over an
     *                 explicit row list this is "these rows of A X"; all other rows of Y keep their contents. */
    const uint8_t* x_row_mask; int32_t x_mask_active; uint8_t* y_row_flag; const uint8_t* z_row_flag; const uint8_t* y_row_gate;
    const uint8_t* y_row_needed; int32_t rows_listed_only;
    /* SLICE-RANGED mask with a DEVICE stamp (the training step's in-place side product dU_cat += A_iu^T dI_cat: the attribute slices of
     * dI_cat are zero outside the rows of the batch's items, which the loss launch stamps - llmrec_bpr_multi_select_bwd_f32).
     *   x_mask_stamp  NULL = none of this. Else a device counter: the active byte of x_row_mask is LLMREC_ROW_STAMP(*x_mask_stamp), read
     *                 by the kernel, so it may change between replays of a captured launch (x_mask_active is ignored);
     *   mask_from_slice (0 .. d / slice_width; slice_width = 0 counts as one slice): in the (row, slice) tasks with slice >=
     *                 mask_from_slice, rows of X whose x_row_mask byte differs from the stamp are PROMISED all-zero in that slice's columns
     *                 and are not read there (they may hold anything); tasks of lower slices run exactly as without a mask.
     * The result equals the unmasked product on the promised zeros bit for bit: the skipped addends are w * (+0) on an accumulator that
     * starts at +0. IN-PLACE SKIP: when the product is the in-place accumulate (Z aliases Y with ldz = ldy, alpha = 1, op NONE, no
     * post_scale), a masked task whose row has no active neighbour neither reads Z nor writes Y - the row keeps its bits (the unmasked
     * product would turn a -0 of Z into +0, nothing else); rows of the block and split buckets are always computed and written.
     * Excludes y_row_flag, z_row_flag, y_row_gate, y_row_needed, rows_listed_only and the softmax epilogues (LLMREC_EINVAL). Compiled for
     * the pattern-only float4 products weighted by col_scale (val NULL) of 33..64 columns per slice (16 lanes per row) - alone, in
     * llmrec_spmm_multi_f32 (whose other members run unmasked beside it; they must be products of the same family weighted by col_scale
     * alone, without y_row_needed) and as the host of the LLMREC_SPMM_GUEST_LOSSES guest; any
     * other shape, variant, company or guest returns LLMREC_EUNSUPPORTED before anything is launched and the caller issues the unmasked
     * call (which is correct whenever the promised rows really hold zeros). */
    const int32_t* x_mask_stamp; int32_t mask_from_slice;
} llmrec_spmm_epilogue_t;
/* Round 5 - "these rows of A X" with the row list AND its length in device memory (the row-restricted forward of the row-sharded step,
 * without a host read-back: llmrec_amd/dist_fused.py). Pattern-only operands (A = diag(row_scale) P).
 *   llmrec_sort_unique_ids_i32   list[0 .. *n_out) = the distinct ids >= 0 among ids[0 .. n), ascending (n <= LLMREC_SORT_UNIQUE_MAX: one block,
 *                                bitonic network over 32-bit keys in LDS); list holds n entries.
 *   llmrec_spmm_rows_compact_f32 out[j] = row_scale[r_j] * sum_{c in row r_j} X[c] for j < *n_list_dev, r_j = row_list[j]; out[j] = 0 for
 *                                *n_list_dev <= j < capacity (a fixed-size message for the exchange that follows). Long rows are cut into up to
 *                                LLMREC_SPMM_COMPACT_PARTS pieces (one block each, partial sums added in piece order by a second launch:
 *                                deterministic). workspace: llmrec_spmm_rows_compact_workspace_bytes(capacity, d).
 *   llmrec_scatter_set_rows_f32  dst[row_list[j]] = src[j] for j < *n_list_dev. */
#define LLMREC_SORT_UNIQUE_MAX 32768
#define LLMREC_SPMM_COMPACT_PARTS 8
int llmrec_sort_unique_ids_i32(int64_t n, const int64_t* ids, int32_t* list, int32_t* n_out, llmrec_stream_t stream);
int64_t llmrec_spmm_rows_compact_workspace_bytes(int64_t capacity, int32_t d);
int llmrec_spmm_rows_compact_f32(int64_t n_rows, int64_t n_cols, const int32_t* rowptr, const int32_t* colidx, const float* row_scale,
                                 const float* X, int64_t ldx, int32_t d, const int32_t* row_list, const int32_t* n_list_dev, int32_t capacity,
                                 float* out, int64_t ldo, void* workspace, int64_t workspace_bytes, llmrec_stream_t stream);
int llmrec_scatter_set_rows_f32(int32_t capacity, const int32_t* row_list, const int32_t* n_list_dev, int32_t d, const float* src, int64_t lds,
                                float* dst, int64_t ldd, llmrec_stream_t stream);
/* flags[ids[j]] = value for j < n (ids[j] < 0 skipped): marks the rows a batch touches (x_row_mask / z_row_flag above) */
int llmrec_mark_rows_u8(int64_t n, const int64_t* ids, int32_t value, uint8_t* flags, llmrec_stream_t stream);
/* flags[c] = value for every column c of the CSR rows ids[j], j < n (ids[j] < 0 skipped): the rows of the transposed operand that have
 * one of the listed rows as a neighbour - with the by-item CSR and the batch's items: the users whose gradient the items' gradient reaches */
int llmrec_mark_neighbours_u8(int64_t n, const int64_t* ids, const int32_t* rowptr, const int32_t* colidx, int32_t value, uint8_t* flags,
                              llmrec_stream_t stream);
/* The user rows a training step's batch reaches, as an ascending row list (two launches, no host read-back - capturable): the batch's
 * users and every user adjacent to one of the batch's positive / negative items. These are the only rows in which the gradient of the
 * attribute streams' projected features is non-zero (reference Models.py:160-163 + main.py:249-254: an attribute stream reaches the loss
 * through the fused embeddings and the BPR terms of the batch's rows; its gradient travels back through A_iu^T from the batch's items) -
 * the row list of llmrec_wgrad_problem_t. users / pos / neg: the batch (int64, B_cap entries, the first *n_valid valid; n_valid NULL =
 * all; negative ids skipped); item_rowptr / item_colidx: the by-item CSR (row = item, columns = its users); flags: n_users bytes of
 * scratch, ALL-ZERO on entry and left all-zero; row_list: n_users + 32 entries; n_rows: device scalar. */
int llmrec_batch_reach_rows(int64_t n_users, int64_t n_items, const int64_t* users, const int64_t* pos, const int64_t* neg, int32_t B_cap,
                            const int32_t* n_valid, const int32_t* item_rowptr, const int32_t* item_colidx, uint8_t* flags,
                            int32_t* row_list, int32_t* n_rows, llmrec_stream_t stream);

/* counts_host[0..3] = n_wave_rows, n_block_rows, n_split_rows, n_segments (synchronises the stream). */
int llmrec_spmm_plan_count(int64_t n_rows, const int32_t* rowptr, int32_t t_wave, int32_t t_block, int32_t segment,
                           int32_t* scratch4 /* device, 4 ints */, int32_t* counts_host, llmrec_stream_t stream);
int llmrec_spmm_plan_fill(int64_t n_rows, const int32_t* rowptr, int32_t t_wave, int32_t t_block, int32_t segment,
                          int32_t* scratch4, int32_t* wave_rows, int32_t* block_rows, int32_t* split_rows,
                          int32_t* split_seg_begin, int32_t* seg_split, llmrec_stream_t stream);

/* p_colidx[p_rowptr[s] + j] = colidx[rowptr[perm[s]] + j]: the CSR with its rows stored in the order perm (p_rowptr = the prefix sums of the
 * permuted row lengths, computed by the caller). One lane group per row. */
int llmrec_csr_permute_rows(int64_t n_rows, const int32_t* rowptr, const int32_t* colidx, const int32_t* perm, const int32_t* p_rowptr,
                            int32_t* p_colidx, llmrec_stream_t stream);

int llmrec_spmm_f32(int64_t n_rows, int64_t n_cols,
                    const int32_t* rowptr, const int32_t* colidx, const float* val,
                    const float* row_scale, const float* col_scale,
                    const float* X, int64_t ldx, float* Y, int64_t ldy, int32_t d, int32_t slice_width,
                    const llmrec_spmm_plan_t* plan_host, float* partials,
                    const llmrec_spmm_epilogue_t* epilogue_host /* NULL = none */, llmrec_stream_t stream);

/* MIXED-PRECISION PROPAGATION (opt-in: llmrec_amd/dist_fused.py, gather_dtype = "bf16"): the product that gathers BF16 rows. At scale the
 * SpMM is bound by the fabric's rate for random row gathers, and a d = 64 row is two 128-B lines in fp32 but one in bf16. Only the gathered
 * operand is narrow: indices, weights, accumulation, the epilogue's operands and Y are fp32, as in llmrec_spmm_f32.
 *   llmrec_rows_to_bf16     Xb[r] = RNE_bf16(row_scale[r] * X[r]) (row_scale NULL = none): one dense pass, the bf16 shadow of an fp32 tensor
 *                           (round to nearest even, NaN -> quiet NaN: torch's float -> bfloat16). Any d and ld; 16-byte rows of X and 8-byte
 *                           rows of Xb take the vector path.
 *   llmrec_spmm_xbf16_f32   Y = post_scale . op(alpha Z + diag(row_scale) (P (.) val) diag(col_scale) widen(Xb)) - every argument but Xb / Yb
 *                           as in llmrec_spmm_f32, without column slices. The fp32 vector families' lanes per row (d <= 16 / 32 / 64 / 128 /
 *                           256) each load their four columns as ONE 8-byte access and widen them by a 16-bit shift; buckets, plans (permuted
 *                           CSR included) and summation trees are those of llmrec_spmm_f32, so the result is BIT-IDENTICAL to llmrec_spmm_f32
 *                           on the fp32 tensor widen(Xb).
 *                           Yb (NULL = none): Yb[r] = RNE_bf16(Y[r]) of the FINISHED row - after the epilogue and post_scale; for split rows
 *                           by the finalize launch - the shadow the next product of a chain gathers from. Yb must not overlap Xb.
 *                           Supported: d % 4 == 0, d <= 256; ldxb % 4 == 0 and Xb 8-byte aligned; Yb rows 8-byte aligned; Y, Z, S, partials as
 *                           the vector path of llmrec_spmm_f32 needs them (16-byte rows); epilogue ops NONE / SOFTMAX / SOFTMAX_BWD with
 *                           alpha, Z (may alias Y), S, post_scale. LLMREC_EUNSUPPORTED for any other d and for an epilogue with x_row_mask,
 *                           y_row_flag, z_row_flag, y_row_gate, y_row_needed, rows_listed_only or x_mask_stamp (masked products gather few
 *                           rows and stay fp32); LLMREC_EINVAL for bad arguments (null pointers, ld < d, misaligned rows, a bad plan) -
 *                           either way before anything is launched, nothing written. No grouped, guest or hosted form. */
int llmrec_rows_to_bf16(int64_t n_rows, int32_t d, const float* row_scale /* NULL = none */,
                        const float* X, int64_t ldx, uint16_t* Xb, int64_t ldxb, llmrec_stream_t stream);
int llmrec_spmm_xbf16_f32(int64_t n_rows, int64_t n_cols, const int32_t* rowptr, const int32_t* colidx, const float* val,
                          const float* row_scale, const float* col_scale,
                          const uint16_t* Xb, int64_t ldxb,            /* the gathered operand: bf16 rows */
                          float* Y, int64_t ldy,
                          uint16_t* Yb, int64_t ldyb,                  /* NULL, or: Yb[r] = RNE_bf16(Y[r]) of the FINISHED row */
                          int32_t d, const llmrec_spmm_plan_t* plan_host, float* partials,
                          const llmrec_spmm_epilogue_t* epilogue_host /* NULL = none */, llmrec_stream_t stream);

/* Independent products in ONE launch (the latency-bound step: each product alone leaves most CUs idle). Each llmrec_spmm_problem_t carries
 * exactly the arguments of one llmrec_spmm_f32 call and is checked like one; the problems' blocks follow each other in the given order
 * (longest first keeps the tail short), and problems with split rows share one finalize launch after the main one. Every row keeps its
 * summation tree: results are bit-identical to separate calls. n = 1 is llmrec_spmm_f32. Returns LLMREC_EUNSUPPORTED (nothing launched)
 * if the problems do not all resolve to the same kernel instance (width class, vector loads, weighted, masked) - the caller
 * then issues separate calls - and LLMREC_EINVAL if the output (Y or partials) of one problem overlaps X, Y, Z, S or the partials of
 * another. Empty problems (n_rows = 0 or d = 0) are skipped. */
#define LLMREC_SPMM_MAX_PROBLEMS 4
typedef struct {
    int64_t n_rows, n_cols;
    const int32_t* rowptr; const int32_t* colidx; const float* val;
    const float* row_scale; const float* col_scale;
    const float* X; int64_t ldx; float* Y; int64_t ldy; int32_t d; int32_t slice_width;
    const llmrec_spmm_plan_t* plan; float* partials;
    const llmrec_spmm_epilogue_t* epilogue;      /* NULL = none */
} llmrec_spmm_problem_t;
int llmrec_spmm_multi_f32(int32_t n, const llmrec_spmm_problem_t* problems, llmrec_stream_t stream);

/* llmrec_spmm_multi_f32 with a GUEST: one short, independent launch of the step whose blocks run as the FIRST blocks of the grouped
 * SpMM launch (they start first; the problems' block ranges follow, shifted by the guest's block count) instead of holding the stream
 * alone while most CUs idle. The guest descriptor is tagged and carries exactly the arguments of the guest's stand-alone entry point,
 * which are checked as that entry point checks them:
 *   LLMREC_SPMM_GUEST_SAMPLER     llmrec_sample_batch_wide               (512-thread blocks: ceil(B / 512) + 1)
 *   LLMREC_SPMM_GUEST_PLAN_REACH  llmrec_bpr_scatter_plan_reach_mark     (32 keys / 8 marking wavefronts per block; 16 B_max B of LDS)
 *   LLMREC_SPMM_GUEST_LOSSES      llmrec_bpr_multi_losses_assemble_f32   (one block: 8 wavefronts take two of the trees each)
 * Every SpMM result and every guest output is bit for bit that of the separate calls: a row's, key's, slot's or tree's work and its order
 * of additions do not depend on the block that holds it. No block waits for another one. The caller guarantees what it guarantees for
 * two launches that may overlap: the guest reads nothing a problem writes and writes nothing a problem reads or writes.
 * Compiled for the step's instance only - 16 lanes per row, float4, d (or the slice width) in 33..64, unmasked, unweighted or weighted
 * (and, for the LOSSES guest, the slice-masked weighted product: llmrec_spmm_epilogue_t.x_mask_stamp).
 * Returns LLMREC_EUNSUPPORTED, BEFORE anything is launched, for every other group (also one llmrec_spmm_multi_f32 would refuse, or
 * without a non-empty problem), for a guest its body cannot take (B_max > LLMREC_BPR_MAX_B, an empty capacity) and for a plan whose LDS
 * would cost the launch its occupancy (B_max > LLMREC_SPMM_GUEST_MAX_PLAN_B): the caller then issues the separate calls. n = 1 hosts the
 * guest in a single product. Problems with split rows keep their finalize launch, without guest blocks. */
#define LLMREC_SPMM_GUEST_SAMPLER 1
#define LLMREC_SPMM_GUEST_PLAN_REACH 2
#define LLMREC_SPMM_GUEST_LOSSES 3
#define LLMREC_SPMM_GUEST_MAX_PLAN_B 3072
typedef struct {                                   /* llmrec_sample_batch_wide */
    uint64_t seed; uint64_t* step_dev; int64_t n_exist_users; const int64_t* exist_users;
    int64_t n_items; const int32_t* train_rowptr; const int32_t* train_colidx;
    int32_t B_global; int32_t slice_begin; int32_t B; int32_t n_aug;
    const int64_t* aug_pos; const int64_t* aug_neg;
    int64_t* users; int64_t* pos; int64_t* neg; int32_t* n_valid_dev; int32_t* ticket;
} llmrec_guest_sampler_t;
typedef struct {                                   /* llmrec_bpr_scatter_plan_reach_mark */
    const int64_t* users; const int64_t* pos; const int64_t* neg; int32_t B_max; const int32_t* n_valid_dev;
    uint64_t* plan; int64_t n_users; int64_t n_items; const int32_t* item_rowptr; const int32_t* item_colidx; uint8_t* flags;
} llmrec_guest_plan_reach_t;
typedef struct {                                   /* llmrec_bpr_multi_losses_assemble_f32 */
    int32_t n_problems; int32_t B_max; const int32_t* n_valid_dev; double remember_rate; float decay; float batch_size_flag;
    float* out; float* saved; const float* w_mf_host; const float* sumsq_partial; int32_t n_partial; float feat_reg_coef;
    float* scal4; double* running_sums3;
} llmrec_guest_losses_t;
typedef struct {
    int32_t kind;                                  /* LLMREC_SPMM_GUEST_* */
    union { llmrec_guest_sampler_t sampler; llmrec_guest_plan_reach_t plan_reach; llmrec_guest_losses_t losses; } u;
} llmrec_spmm_guest_t;
int llmrec_spmm_multi_guest_f32(int32_t n, const llmrec_spmm_problem_t* problems, const llmrec_spmm_guest_t* guest, llmrec_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * R4  side-feature projection            replaces nn.Linear forward / weight-grad
 *                                        (reference Models.py:30-37,145-150; aten::addmm, aten::mm)
 * Y[M x N] = X[M x K] * W[N x K]^T + b     (fp32 MFMA v_mfma_f32_16x16x4_f32, exact fp32)
 * dW[N x K] (+)= dY[M x N]^T * X[M x K],  db[N] (+)= column sums of dY.  The inputs X are
 * constants in the reference, so no dX is ever needed.
 * N must be a multiple of 16 and <= 128; K a multiple of 4.
 * ------------------------------------------------------------------------------------------ */
int llmrec_linear_fwd_f32(int64_t M, int32_t N, int32_t K, const float* X, int64_t ldx,
                          const float* W, int64_t ldw, const float* bias,
                          float* Y, int64_t ldy, llmrec_stream_t stream);
/* Several projections in one launch (the reference runs 8 per forward, Models.py:145-150):
 * Y_p = X_p W_p^T + b_p with a common N <= 64. Y_p may be a column slice of a wider buffer (ldy). */
#define LLMREC_LINEAR_MAX_PROBLEMS 8
typedef struct {
    const float* X; int64_t ldx; int64_t M; int32_t K;
    const float* W; int64_t ldw; const float* bias;
    float* Y; int64_t ldy;
    const float* bias_scale;   /* [M] or NULL (= all ones): Y[r] = X[r] W^T + bias_scale[r] * bias. With X = A F (a constant feature
                                  matrix propagated once through a constant adjacency) and bias_scale = the row sums of A this is
                                  A (F W^T + 1 b^T), i.e. projection + propagation (reference Models.py:145-157) as ONE product */
} llmrec_linear_problem_t;
int llmrec_linear_fwd_grouped_f32(int32_t n_problems, const llmrec_linear_problem_t* problems_host, int32_t N,
                                  llmrec_stream_t stream);
/* Weight gradient of one Linear fed by several (dY_p, X_p) pairs - the reference's shared
 * item_trans receives 5 per step (Models.py:150): dW (+)= sum_p dY_p^T X_p, db (+)= sum_p colsum(dY_p).
 * Workspace: llmrec_linear_wgrad_workspace_bytes(sum_p M_p, N, K). */
typedef struct { const float* dY; int64_t lddy; const float* X; int64_t ldx; int64_t M;
                 const float* db_row_weight;   /* [M] or NULL (= ones): db (+)= sum_r db_row_weight[r] dY[r] - the bias gradient of a projection
                                                  with llmrec_linear_problem_t.bias_scale (bf16x3, N = 64, K % 128 == 0 only) */
                 /* ROW LIST (llmrec_linear_wgrad_multi_* with every K % 128 == 0 only; NULL elsewhere): the rows of dY that can be non-zero.
                  * A training step's dY is exactly zero outside the rows its batch reaches (llmrec_batch_reach_rows), and a zero row adds
                  * nothing to dY^T X: the kernel streams the LISTED rows of dY and X only. Contract: row_list = device int32 ids, ascending,
                  * distinct, < M, readable up to n_rows rounded up to 16 entries (+ 16); every row of dY NOT listed is all-zero (it is
                  * never read; a non-zero one would be silently dropped); n_rows = device scalar (<= M), read by the kernel, so the list
                  * can change between replays of a captured launch. rows_expected (host, 0 = M) sizes the launch geometry: the problem
                  * gets ceil(rows_expected / slab) slabs, which the kernel re-cuts into equal pieces of the actual n_rows - a poor
                  * guess costs balance, never correctness. Deterministic; equal to the dense launch up to fp32 summation order. */
                 const int32_t* row_list; const int32_t* n_rows; int64_t rows_expected;
} llmrec_wgrad_problem_t;
int llmrec_linear_wgrad_grouped_f32(int32_t n_problems, const llmrec_wgrad_problem_t* problems_host, int32_t N, int32_t K,
                                    float* dW, int64_t lddw, float* db, int32_t accumulate,
                                    void* workspace, int64_t workspace_bytes, llmrec_stream_t stream);
/* Same contract, split-precision arithmetic (three-term bf16 split of both operands, six bf16 MFMAs per tile pair,
 * fp32 accumulate: fp32-roundoff-class error, bound by the X stream from HBM instead of the fp32 matrix pipe).
 * Shapes outside the fast path (N % 64, K % 64, 16-byte aligned rows) run the exact fp32 kernel. */
int llmrec_linear_wgrad_grouped_bf16x3(int32_t n_problems, const llmrec_wgrad_problem_t* problems_host, int32_t N, int32_t K,
                                       float* dW, int64_t lddw, float* db, int32_t accumulate,
                                       void* workspace, int64_t workspace_bytes, llmrec_stream_t stream);
/* The weight gradients of several Linears (targets) in ONE launch + one reduction launch, split-precision arithmetic as above:
 * target t has its own K, dW, db and (dY_p, X_p) pairs; N is common. All targets are cut into slabs of one length, chosen so
 * that the launch is whole rounds of equal blocks (three back-to-back launches each pay their own ramp-up and ragged last
 * round). Fast path only - N % 64 == 0, K_t % 64 == 0, non-empty problems with 16-byte aligned rows and byte offsets below
 * 2^32 - otherwise LLMREC_EUNSUPPORTED (workspace query: -1) and the caller issues llmrec_linear_wgrad_grouped_bf16x3 per
 * target. Deterministic (fixed slab order); the slab length differs from the single-target launches', so the sums are
 * equal to those only up to fp32 rounding. */
#define LLMREC_WGRAD_MAX_TARGETS 4
typedef struct { int32_t n_problems; const llmrec_wgrad_problem_t* problems; int32_t K; float* dW; int64_t lddw; float* db; int32_t accumulate;
                 int32_t block_budget;   /* read from targets[0] only: lay the launch out as whole rounds of this many blocks (0 = 256, one block per
                                            CU). A budget below 256 leaves CUs to kernels on other streams: a block of this launch owns its CU's
                                            whole register file, so whatever runs beside a 256-block round waits for it to drain */
} llmrec_wgrad_target_t;
int64_t llmrec_linear_wgrad_multi_workspace_bytes(int32_t n_targets, const llmrec_wgrad_target_t* targets_host, int32_t N);
int llmrec_linear_wgrad_multi_bf16x3(int32_t n_targets, const llmrec_wgrad_target_t* targets_host, int32_t N,
                                     void* workspace, int64_t workspace_bytes, llmrec_stream_t stream);
/* llmrec_linear_wgrad_multi_bf16x3 with the AdamW update of every target's W and b inside the reduction launch (the arithmetic of
 * llmrec_adamw_multi_f32, element by element, on the gradient that launch has just summed and stored: parameters, moments and
 * gradients come out bit-identical to the two calls in sequence). A fused training step ends on this launch instead of
 * reduction -> update. updates_host[t]: W / b (the parameters dW / db are the gradients of; b, m_b, v_b NULL when the target has no
 * db), their moments, g_scale as in llmrec_adamw_tensor_t; W and dW contiguous (lddw == K); state3 = the device state of
 * llmrec_adamw_advance. */
typedef struct { float* W; float* m_W; float* v_W; float* b; float* m_b; float* v_b; float g_scale; } llmrec_wgrad_update_t;
int llmrec_linear_wgrad_multi_adamw_bf16x3(int32_t n_targets, const llmrec_wgrad_target_t* targets_host, int32_t N,
                                           void* workspace, int64_t workspace_bytes, const llmrec_wgrad_update_t* updates_host,
                                           const float* state3, float lr, float beta1, float beta2, float eps, float weight_decay,
                                           llmrec_stream_t stream);
/* llmrec_linear_wgrad_multi_adamw_bf16x3 hosting ONE independent SpMM (a problem as llmrec_spmm_multi_f32 takes it) in the CUs its
 * weight-gradient launch leaves free: a block of that launch owns a whole CU, and a block_budget below the device's CU count lays it
 * out for fewer blocks than CUs. The launch becomes n_cu blocks - the weight gradient's wg_blocks, unchanged and placed first, then
 * n_guest = n_cu - wg_blocks guests that run the product's blocks persistently (guest g: blocks g, g + n_guest, ...); the reduction +
 * AdamW launch follows unchanged. n_cu = the device's CU count, passed by the caller (no device query here). The product depends on
 * nothing either launch computes and no block waits for another. Gradients, parameters, moments and the product's Y are bit-identical to
 * llmrec_linear_wgrad_multi_adamw_bf16x3 and llmrec_spmm_f32 in either order: the slab length does not depend on the guest, and the
 * product's 256-thread blocks keep every row's summation tree. Compiled for the 128-wide organisation (every K % 128 == 0) at N = 64 and
 * the unmasked float4 product of 33..64 columns weighted by col_scale alone, with or without the init term alpha Z (LLMREC_SPMM_EPI_NONE),
 * without val, slices, split rows, softmax epilogue, post_scale or row restriction. LLMREC_EUNSUPPORTED before anything is launched -
 * the caller then issues the two separate calls - for anything else, when wg_blocks >= n_cu (no free CU), when the product's Y overlaps
 * anything the two launches read or write (every dY, X, row list and count, the workspace, dW / db, parameters, moments, state3) and
 * when the product's X or Z overlaps anything they write. */
int llmrec_linear_wgrad_multi_adamw_host_spmm_bf16x3(int32_t n_targets, const llmrec_wgrad_target_t* targets_host, int32_t N,
                                                     void* workspace, int64_t workspace_bytes, const llmrec_wgrad_update_t* updates_host,
                                                     const float* state3, float lr, float beta1, float beta2, float eps, float weight_decay,
                                                     const llmrec_spmm_problem_t* spmm, int32_t n_cu, llmrec_stream_t stream);
/* Same contract, split precision: each fp32 operand = exact sum of three bf16 numbers, product by the
 * six bf16 MFMAs (v_mfma_f32_16x16x32_bf16, fp32 accumulate) whose terms are >= 2^-24 relative.
 * fp32-roundoff-class error (not the bit-identical fma chain); 3/8 of the fp32 matrix time, so the
 * kernel becomes HBM-bound on the X stream. */
int llmrec_linear_fwd_grouped_bf16x3(int32_t n_problems, const llmrec_linear_problem_t* problems_host, int32_t N,
                                     llmrec_stream_t stream);
/* llmrec_linear_fwd_grouped_bf16x3 hosting ONE independent SpMM (a problem as llmrec_spmm_multi_f32 takes it) as the TRAILING blocks
 * of its launch: grid = the projection's work units + the product's blocks. Once the launch has more units than the device has block
 * slots, its last round leaves slots empty; the product's blocks land there. The product depends on nothing the launch computes
 * (spmm->X and spmm->Y overlap no projection's Y) and no block waits for another. The projections' Y and the product's Y are
 * bit-identical to llmrec_linear_fwd_grouped_bf16x3 followed by llmrec_spmm_f32: the product's 256-thread blocks keep every row's
 * summation tree. Compiled for the projection's <N = 49..64, 128-row units, 32-aligned K> instance and the unweighted, unmasked float4
 * product of 33..64 columns without slices, split rows or epilogue. Anything else: LLMREC_EUNSUPPORTED before anything is launched,
 * and the caller issues the two separate calls. */
int llmrec_linear_fwd_grouped_host_spmm_bf16x3(int32_t n_problems, const llmrec_linear_problem_t* problems_host, int32_t N,
                                               const llmrec_spmm_problem_t* spmm, llmrec_stream_t stream);
int64_t llmrec_linear_wgrad_workspace_bytes(int64_t M, int32_t N, int32_t K);
int llmrec_linear_wgrad_f32(int64_t M, int32_t N, int32_t K, const float* dY, int64_t lddy,
                            const float* X, int64_t ldx, float* dW, int64_t lddw, float* db,
                            int32_t accumulate, void* workspace, int64_t workspace_bytes,
                            llmrec_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * R3  last-layer row softmax + mean over the L+1 layer outputs
 *                                        replaces nn.Softmax(dim=-1) and stack+mean
 *                                        (reference Models.py:176-177,185-186)
 * ------------------------------------------------------------------------------------------ */
int llmrec_softmax_rows_fwd_f32(int64_t rows, int32_t d, const float* Z, int64_t ldz,
                                float* Y, int64_t ldy, llmrec_stream_t stream);
/* dZ = Y (.) (dY - <dY, Y>_row) */
int llmrec_softmax_rows_bwd_f32(int64_t rows, int32_t d, const float* Y, int64_t ldy,
                                const float* dY, int64_t lddy, float* dZ, int64_t lddz,
                                llmrec_stream_t stream);
/* dZ = softmax_bwd(Y, alpha * dY): the scaling of the incoming gradient (the "+ mean term" factor 1 / (L + 1) of the ID chain) in the
 * same pass; alpha = 1 is llmrec_softmax_rows_bwd_f32 bit for bit. */
int llmrec_softmax_rows_bwd_scaled_f32(int64_t rows, int32_t d, float alpha, const float* Y, int64_t ldy, const float* dY, int64_t lddy,
                                       float* dZ, int64_t lddz, llmrec_stream_t stream);
/* The same for the listed rows only, with a per-row scale of the result: dZ[r] = post_scale[r] * softmax_bwd(Y[r], alpha * dY[r]) for
 * r = ids[j], j < n (ids[j] < 0 skipped; duplicates write the same values). The other rows of dZ are not touched: the first gradient of
 * the row-sharded step's backward is needed (and, behind an x_row_mask, read) only in the rows of the batch's items. */
int llmrec_softmax_rows_bwd_listed_f32(int64_t n, const int64_t* ids, int32_t d, float alpha, const float* Y, int64_t ldy,
                                       const float* dY, int64_t lddy, const float* post_scale, float* dZ, int64_t lddz,
                                       llmrec_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * R6  fusion  out = scale * sum_t mean_terms[t] + sum_t rates[t] * normalize(terms[t])
 *                                        replaces torch.mean(torch.stack(..)) + the 16
 *                                        F.normalize / scaled-add calls (reference Models.py:185-197)
 * normalize(x) = x / max(||x||_2, 1e-12) row-wise. Term pointer/ld/rate tables live on the HOST
 * (<= LLMREC_MAX_TERMS each) and are passed by value to the kernel.
 * bwd: d_mean (shared by all mean terms) = scale * dOut is NOT written (the caller scales);
 *      d_terms[t] (+)= rates[t] * (dOut - n <n, dOut>) / max(||x||, 1e-12)   [+ reg_two_coef * x for t < n_reg_terms]
 * ------------------------------------------------------------------------------------------ */
#define LLMREC_MAX_TERMS 12
int llmrec_fuse_fwd_f32(int64_t rows, int32_t d, float mean_scale,
                        int32_t n_mean, const float* const* mean_terms_host, const int64_t* mean_ld_host,
                        int32_t n_norm, const float* const* norm_terms_host, const int64_t* norm_ld_host,
                        const float* rates_host, float* out, int64_t ldo, llmrec_stream_t stream);
int llmrec_fuse_bwd_f32(int64_t rows, int32_t d, const float* dOut, int64_t lddo,
                        int32_t n_norm, const float* const* norm_terms_host, const int64_t* norm_ld_host,
                        const float* rates_host, float* const* d_terms_host, const int64_t* d_ld_host,
                        int32_t accumulate, int32_t n_reg_terms, float reg_two_coef, llmrec_stream_t stream);
/* The same with a SOURCE per term: d_terms[t] = src_terms[t] (or 0 where src_terms[t] is NULL) + the term's gradient, written
 * without reading d_terms. With the loss backward scattering into separate, otherwise all-zero source buffers
 * (llmrec_bpr_multi_bwd_f32) and llmrec_bpr_multi_zero_rows_f32 clearing the touched rows afterwards, a training step needs no
 * dense memset of its gradient buffers. */
int llmrec_fuse_bwd_src_f32(int64_t rows, int32_t d, const float* dOut, int64_t lddo,
                            int32_t n_norm, const float* const* norm_terms_host, const int64_t* norm_ld_host,
                            const float* rates_host, float* const* d_terms_host, const int64_t* d_ld_host,
                            const float* const* src_terms_host, const int64_t* src_ld_host,
                            int32_t n_reg_terms, float reg_two_coef, llmrec_stream_t stream);
/* The user-side and the item-side fusion (or fusion backward, llmrec_fuse_bwd_src_f32 semantics) of one step as ONE launch
 * (n_problems <= 2; the two row ranges are independent): on two streams each launch paid a cross-queue fork and join for
 * 15 - 26 us of work (reference Models.py:188-197 for users and items). */
typedef struct {
    int64_t rows; float mean_scale;
    int32_t n_mean; const float* const* mean_terms; const int64_t* mean_ld;
    int32_t n_norm; const float* const* norm_terms; const int64_t* norm_ld; const float* rates;
    float* out; int64_t ldo;
} llmrec_fuse_fwd_problem_t;
int llmrec_fuse_fwd_multi_f32(int32_t n_problems, const llmrec_fuse_fwd_problem_t* problems_host, int32_t d, llmrec_stream_t stream);
/* The same launch, which ALSO leaves the sum of squares of the first n_sumsq_terms norm terms of every problem (the image / text streams the
 * feature regulariser of reference main.py:151-156 sums: the kernel holds those rows and their squared norms in registers anyway) as one
 * partial sum per block: sumsq_partial[0 .. *n_partial_host) (fixed block partition, fixed in-block tree: deterministic). *n_partial_host is
 * written on the HOST at call time (a pure function of the problems' row counts, <= partial_capacity or the call fails); the consumer is
 * llmrec_bpr_multi_losses_assemble_f32. Replaces the four llmrec_sumsq_f32 launches of a step. */
int llmrec_fuse_fwd_multi_sumsq_f32(int32_t n_problems, const llmrec_fuse_fwd_problem_t* problems_host, int32_t d, int32_t n_sumsq_terms,
                                    float* sumsq_partial, int32_t partial_capacity, int32_t* n_partial_host, llmrec_stream_t stream);
/* The same launch with ONE more block in front, which does the second half of llmrec_batch_reach_rows: it turns the byte flags
 * (n_users bytes, 16-byte aligned and readable up to n_users rounded up to 16) into the ascending row_list (n_users + 32 entries, the
 * same padding entries), writes *n_rows and leaves the flags all-zero. The fusion's outputs and partial sums are those of
 * llmrec_fuse_fwd_multi_sumsq_f32, bit for bit; the list's reader runs at the far end of the step, so the compaction hides behind the
 * fusion's blocks. Only the float4 row family (d % 4 == 0, 16-byte aligned rows, d <= 512) is compiled: any other shape returns
 * LLMREC_EUNSUPPORTED before anything is launched, and the caller issues the two separate calls. */
int llmrec_fuse_fwd_multi_sumsq_compact_f32(int32_t n_problems, const llmrec_fuse_fwd_problem_t* problems_host, int32_t d, int32_t n_sumsq_terms,
                                            float* sumsq_partial, int32_t partial_capacity, int32_t* n_partial_host,
                                            int64_t n_users, uint8_t* flags, int32_t* row_list, int32_t* n_rows, llmrec_stream_t stream);
typedef struct {
    int64_t rows; const float* dOut; int64_t lddo;
    int32_t n_norm; const float* const* norm_terms; const int64_t* norm_ld; const float* rates;
    float* const* d_terms; const int64_t* d_ld;
    const float* const* src_terms; const int64_t* src_ld;      /* src_terms[t] may be NULL (= 0) */
    int32_t n_reg_terms; float reg_two_coef;
    const uint8_t* row_flags;   /* [rows] or NULL. A row whose flag is not ACTIVE (see LLMREC_ROW_STAMP below) PROMISES that dOut[r] and every
                                   source row r are all-zero (a row no sample of the batch touched - llmrec_bpr_multi_select_bwd_f32 stamps the
                                   rows it touches): the kernel then writes the regulariser's term for the first n_reg_terms streams and zeros
                                   for the others without reading anything else - the same bits, ~half the traffic at 10 % touched rows */
    const int32_t* row_stamp;   /* device counter that defines ACTIVE, or NULL (active = non-zero flag) */
    int32_t zero_skip_from_term; /* 0 = none. Else (>= n_reg_terms, needs row_flags): in a row that is not ACTIVE the terms at or beyond this index are
                                   NOT WRITTEN (they would be zeros; the rows keep stale contents) - for terms whose only reader skips the
                                   rows that are not ACTIVE by the same flags and stamp (llmrec_spmm_epilogue_t.x_mask_stamp) */
} llmrec_fuse_bwd_problem_t;
int llmrec_fuse_bwd_src_multi_f32(int32_t n_problems, const llmrec_fuse_bwd_problem_t* problems_host, int32_t d, llmrec_stream_t stream);

/* n_reg_terms / reg_two_coef: the first n_reg_terms terms additionally receive reg_two_coef * x - the gradient of a
 * sum-of-squares regulariser coef * sum x^2 on them (reference main.py:151-156 on the image / text streams), folded in
 * because the kernel has x in registers anyway; pass 0, 0 for the plain backward. */

/* ------------------------------------------------------------------------------------------
 * R7  fused BPR + prune loss             replaces the 3 gathers, mul/sum, logsigmoid, the
 *                                        D2H argsort of prune_loss and its backward
 *                                        (reference main.py:158-165,232-254,330-342)
 * For sample b < B:  s_b = <Eu[u_b], Ei[p_b]> - <Eu[u_b], Ei[q_b]>,  m_b = logsigmoid(s_b + 1e-8)
 * keep = the k = (int)(remember_rate * B) samples with the SMALLEST m_b (ties: lower b first)
 * out[0] = mf  = -(1/k) * sum_keep m_b
 * out[1] = emb = decay / batch_size_flag * (1/(2 Su + 1e-8) + 1/(2 Sp + 1e-8) + 1/(2 Sq + 1e-8)),
 *          S* = squared Frobenius norms of the three gathered B x d blocks
 * The forward stores what backward needs (per-sample ds_b, the three norms, and per-sample
 * scratch) in `saved` (LLMREC_BPR_SAVED_FLOATS(B_max) floats). B may come from device memory (n_valid_dev != NULL) so a captured graph can
 * replay with a varying number of augmented triples; B_max bounds it (<= LLMREC_BPR_MAX_B).
 * ------------------------------------------------------------------------------------------ */
#define LLMREC_BPR_MAX_B 4096
#define LLMREC_BPR_MAX_PROBLEMS 8
#define LLMREC_BPR_SAVED_FLOATS(B) (6 * (B) + 8)   /* floats of `saved` per problem */
int llmrec_bpr_prune_fwd_f32(const float* Eu, int64_t ldu, const float* Ei, int64_t ldi, int32_t d,
                             const int64_t* users, const int64_t* pos, const int64_t* neg,
                             int32_t B_max, const int32_t* n_valid_dev,
                             double remember_rate, float decay, float batch_size_flag,
                             float* out2, float* saved, llmrec_stream_t stream);
/* User-sharded batch: every rank holds B_local samples of a global batch of
 * global_B. Pass 1 (scores_only = 1) writes the local m_b to saved[0..B_local) and the local
 * squared norms per sample to the scratch part of saved (m_b at saved[B_local + 4 + b]); the
 * host all-gathers the m_b (RCCL) and calls
 * pass 2 with them: selection ranks against the GLOBAL batch (ties: lower global index), out2[0]
 * is this rank's share -(1/k) * sum_{kept local} m_b (all-reduce it), and saved is ready for
 * llmrec_bpr_prune_bwd_f32 once saved[B_local..B_local+2] hold the all-reduced norms. */
int llmrec_bpr_prune_fwd_sharded_f32(const float* Eu, int64_t ldu, const float* Ei, int64_t ldi, int32_t d,
                                     const int64_t* users, const int64_t* pos, const int64_t* neg,
                                     int32_t B_local, double remember_rate, float decay, float batch_size_flag,
                                     const float* global_m, int32_t global_B, int32_t my_offset, int32_t scores_only,
                                     float* out2, float* saved, llmrec_stream_t stream);
/* Both single-problem forms above for batches of ANY size up to LLMREC_BPR_WIDE_MAX_B (B_local and global_B): the selection is an
 * exact multi-block radix select (four histogram passes over the order-preserving image of m_b, then the ties at the threshold by
 * global index) instead of rank counting in LDS - same keep set, same `saved` layout and bits, same reduction kernel, so out2 and
 * saved equal the capped entry points' wherever both exist. Integer atomics only, no host synchronisation, no allocation; the
 * launch sequence depends on the host arguments alone (hipGraph-capturable).
 *   global_m == NULL, scores_only = 0   the batch is local (llmrec_bpr_prune_fwd_f32): B from n_valid_dev (may be NULL) or B_local;
 *                                       scores, selection, reduction. my_offset = 0, global_B = 0 or B_local.
 *   scores_only = 1                     pass 1 of the sharded form; no workspace needed.
 *   global_m != NULL, scores_only = 0   pass 2: selection of this rank's B_local samples against the global_B gathered scores at
 *                                       my_offset; out2[0] is this rank's share. n_valid_dev bounds the LOCAL samples only.
 * workspace: llmrec_bpr_prune_wide_workspace_bytes(global_B, or B_local for a local batch) bytes, 4-byte aligned; the entry point's
 * own launches initialise it. Too small: LLMREC_EWORKSPACE; a size above LLMREC_BPR_WIDE_MAX_B: LLMREC_EUNSUPPORTED (the query: -1).
 * The multi-problem entry points below stay capped at LLMREC_BPR_MAX_B (DataParallelStep, the default FusedStep); their *_wide twins
 * further down carry the eight-problem loss segment up to LLMREC_BPR_WIDE_MAX_B. */
#define LLMREC_BPR_WIDE_MAX_B (1 << 22)
int64_t llmrec_bpr_prune_wide_workspace_bytes(int64_t global_B);
int llmrec_bpr_prune_fwd_wide_f32(const float* Eu, int64_t ldu, const float* Ei, int64_t ldi, int32_t d,
                                  const int64_t* users, const int64_t* pos, const int64_t* neg,
                                  int32_t B_local, double remember_rate, float decay, float batch_size_flag,
                                  const float* global_m, int32_t global_B, int32_t my_offset, int32_t scores_only,
                                  float* out2, float* saved, const int32_t* n_valid_dev,
                                  void* workspace, int64_t workspace_bytes, llmrec_stream_t stream);
/* Several (user table, item table) pairs over ONE batch in two launches - the reference computes
 * 8 such losses per step (main.py:232-254). out: [n_problems][2], saved: n_problems blocks of
 * LLMREC_BPR_SAVED_FLOATS(B_max). The backward takes the loss weights from the (host) problem
 * table (g_mf, g_emb) and scatter-adds (deterministically, see llmrec_bpr_scatter_plan) into dEu / dEi, which the caller zero-initialises. */
typedef struct {
    const float* Eu; int64_t ldu; const float* Ei; int64_t ldi;
    float* dEu; int64_t lddu; float* dEi; int64_t lddi;
    float g_mf, g_emb;
} llmrec_bpr_problem_t;
int llmrec_bpr_multi_fwd_f32(int32_t n_problems, const llmrec_bpr_problem_t* problems_host, int32_t d,
                             const int64_t* users, const int64_t* pos, const int64_t* neg,
                             int32_t B_max, const int32_t* n_valid_dev, double remember_rate, float decay,
                             float batch_size_flag, float* out, float* saved, llmrec_stream_t stream);
/* Batch-sharded form of llmrec_bpr_multi_fwd_f32 (data-parallel replicas or user-sharded ranks;
 * SURVEY.md 8(e) "all-gather the B log-sigmoids, select the threshold redundantly"). The global
 * batch is the concatenation of the ranks' valid samples in rank order; prune keeps the
 * k = (int)(remember_rate * B_global) smallest m_b of the GLOBAL batch (ties: lower global index).
 *   phase 1: scores + this rank's gather block -> gather_block[LLMREC_BPR_GATHER_FLOATS(P, B_max)]:
 *            [P][B_max] m_b (+inf beyond n_valid) | [P][4] Su, Sp, Sq, - (local sums) | n_valid as float
 *   (host: all-gather the blocks, RCCL; every rank's B_max must be equal)
 *   phase 2: selection against `gathered` ([n_ranks] blocks, rank_stride floats apart): out[p][0] is
 *            this rank's SHARE of mf_p (sum over ranks = mf_p), out[p][1] = emb_p from the global
 *            norms (identical on every rank); `saved` is then ready for llmrec_bpr_multi_bwd_f32.
 * n_ranks * B_max <= 4 * LLMREC_BPR_MAX_B. */
#define LLMREC_BPR_GATHER_FLOATS(P, B) ((P) * (B) + 4 * (P) + 1)
int llmrec_bpr_multi_fwd_sharded_f32(int32_t n_problems, const llmrec_bpr_problem_t* problems_host, int32_t d,
                                     const int64_t* users, const int64_t* pos, const int64_t* neg,
                                     int32_t B_max, const int32_t* n_valid_dev, double remember_rate, float decay,
                                     float batch_size_flag, int32_t phase, float* gather_block,
                                     const float* gathered, int32_t n_ranks, int64_t rank_stride, int32_t my_rank,
                                     float* out, float* saved, llmrec_stream_t stream);
/* DETERMINISTIC gradient scatter (ABI 6). The reference's backward is index_put(accumulate) on CPU - the rows several samples share
 * are added in one fixed order and same-seed runs agree (main.py:232-254,330-342). Every backward entry point below therefore takes a
 * SCATTER PLAN of the batch instead of adding rows with float atomics:
 *   llmrec_bpr_scatter_plan   plan[0 .. B_max)        = the keys  users[b] << 32 | b                          sorted ascending
 *                             plan[B_max .. 3 B_max)  = the keys  pos[b] << 32 | b  and  neg[b] << 32 | (B_max + b), sorted ascending
 *                             (samples b >= n_valid: id 0xffffffff, at the end), then as int32 runlen[3 B_max]: at the first position of a
 *                             run of equal ids the run's length, 0 elsewhere. One launch (rank counting in LDS, ceil(3 B_max / 16) blocks);
 *                             it depends on the batch only, so a step builds it right behind its sampler, off the critical path.
 * In the backward launch the head of every run of equal ids owns the destination row and adds the run's contributions in ascending
 * problem index, then ascending slot. Problems whose dEu (or dEi) POINTERS are equal share one target (the five attribute problems of a
 * step all scatter into d prof_u): the first of them sums the others' shares; targets must otherwise be disjoint. */
#define LLMREC_BPR_PLAN_WORDS(B) (5 * (B))         /* 64-bit words of `plan`: 3 B keys + 3 B int32 run lengths */
int llmrec_bpr_scatter_plan(const int64_t* users, const int64_t* pos, const int64_t* neg, int32_t B_max, const int32_t* n_valid_dev,
                            uint64_t* plan, llmrec_stream_t stream);
/* llmrec_bpr_scatter_plan AND the marking half of llmrec_batch_reach_rows in ONE launch: the plan's blocks come first, the marking
 * blocks behind them. Both read the batch only and neither reads what the other writes; on one stream the flags then cost no launch of
 * their own. The plan is llmrec_bpr_scatter_plan's; flags (n_users bytes, 16-byte aligned, all-zero on entry) are left as
 * llmrec_batch_reach_rows' first launch leaves them: non-zero at the batch's users and at every user adjacent to one of its valid
 * items. item_rowptr / item_colidx: the by-item CSR. The list is then made by llmrec_fuse_fwd_multi_sumsq_compact_f32 (or any compaction
 * of the flags). B_max > LLMREC_BPR_MAX_B: LLMREC_EUNSUPPORTED, nothing launched. */
int llmrec_bpr_scatter_plan_reach_mark(const int64_t* users, const int64_t* pos, const int64_t* neg, int32_t B_max, const int32_t* n_valid_dev,
                                       uint64_t* plan, int64_t n_users, int64_t n_items, const int32_t* item_rowptr,
                                       const int32_t* item_colidx, uint8_t* flags, llmrec_stream_t stream);
int llmrec_bpr_multi_bwd_f32(int32_t n_problems, const llmrec_bpr_problem_t* problems_host, int32_t d,
                             const int64_t* users, const int64_t* pos, const int64_t* neg,
                             int32_t B_max, const int32_t* n_valid_dev, float decay, float batch_size_flag,
                             const float* saved, const uint64_t* plan, llmrec_stream_t stream);
/* The same step of one LOCAL batch (no gathered layout) with the loss VALUES off the critical path - the fused training step's
 * critical path is scores -> selection -> backward rows instead of scores -> rank -> reduce -> backward:
 *   llmrec_bpr_multi_scores_f32       launch 1: m_b, sigmoid(-x_b) and the per-sample squared norms into `saved`
 *   llmrec_bpr_multi_select_bwd_f32   launch 2 (selection): ranks every sample against the batch in LDS and writes the kept coefficients /
 *                                     values into `saved`; one more block per problem sums the batch's squared norms with the summation
 *                                     tree of the loss launch below (so the bits agree) into saved[B_max .. B_max + 2];
 *                                     launch 3 (backward rows): the deterministic scatter of llmrec_bpr_multi_bwd_f32 through `plan`
 *   llmrec_bpr_multi_losses_f32       any time after launch 2, on any stream: out[p] = {mf_p, emb_p} and the norm / k slots of `saved`
 *                                     (only the logged loss values depend on it)
 * Results: `out`, `saved` and the gradient rows bit-identical to llmrec_bpr_multi_fwd_f32 + llmrec_bpr_multi_bwd_f32. */
/* Row stamps: the rows a batch touches are marked in byte arrays with the value LLMREC_ROW_STAMP(counter) of a device counter that
 * the scores launch advances once per step; consumers (llmrec_fuse_bwd_problem_t.row_flags) treat a
 * row as touched iff its byte equals the current stamp. Nothing ever has to be cleared - a stale byte differs from the current stamp for
 * the next 254 steps, and a false "touched" only costs the general path (same result). */
#define LLMREC_ROW_STAMP(counter) ((uint8_t)((uint32_t)(counter) % 255u + 1u))
int llmrec_bpr_multi_scores_f32(int32_t n_problems, const llmrec_bpr_problem_t* problems_host, int32_t d,
                                const int64_t* users, const int64_t* pos, const int64_t* neg,
                                int32_t B_max, const int32_t* n_valid_dev, float* saved,
                                int32_t* row_stamp /* optional: device counter, += 1 by this launch */, llmrec_stream_t stream);
int llmrec_bpr_multi_select_bwd_f32(int32_t n_problems, const llmrec_bpr_problem_t* problems_host, int32_t d,
                                    const int64_t* users, const int64_t* pos, const int64_t* neg,
                                    int32_t B_max, const int32_t* n_valid_dev, double remember_rate, float decay,
                                    float batch_size_flag, float* saved,
                                    uint8_t* user_row_flags, uint8_t* item_row_flags,   /* optional: [u_b] / [p_b], [q_b] := stamp for b < n_valid */
                                    const int32_t* row_stamp,                           /* optional device counter (NULL: stamp = 1) */
                                    const uint64_t* plan,                               /* llmrec_bpr_scatter_plan of this batch */
                                    llmrec_stream_t stream);
int llmrec_bpr_multi_losses_f32(int32_t n_problems, int32_t B_max, const int32_t* n_valid_dev, double remember_rate, float decay,
                                float batch_size_flag, float* out, float* saved, llmrec_stream_t stream);
/* Round 5 - fewer launches per step:
 * llmrec_bpr_multi_scores_step_f32 = llmrec_bpr_multi_scores_f32 that also BEGINS THE STEP on the device: beside the row stamp it advances
 *   AdamW's step counter / bias corrections (llmrec_adamw_advance on adamw_state3; NULL = leave it) - every AdamW launch of the step is
 *   stream-ordered behind the loss launches anyway;
 * llmrec_bpr_multi_losses_assemble_f32 = llmrec_bpr_multi_losses_f32 (same trees, same bits in out / saved) followed, in the same single-block
 *   launch, by the feature regulariser's value feat_reg = feat_reg_coef * sum(sumsq_partial[0 .. n_partial)) (llmrec_fuse_fwd_multi_sumsq_f32;
 *   fixed-order tree) -> scal4[0] and by llmrec_loss_assemble_f32 mode 0 (scal4[1..3] = loss, mf, emb; running_sums3 += them in double). */
int llmrec_bpr_multi_scores_step_f32(int32_t n_problems, const llmrec_bpr_problem_t* problems_host, int32_t d,
                                     const int64_t* users, const int64_t* pos, const int64_t* neg,
                                     int32_t B_max, const int32_t* n_valid_dev, float* saved, int32_t* row_stamp,
                                     float* adamw_state3, float lr, float beta1, float beta2, llmrec_stream_t stream);
int llmrec_bpr_multi_losses_assemble_f32(int32_t n_problems, int32_t B_max, const int32_t* n_valid_dev, double remember_rate, float decay,
                                         float batch_size_flag, float* out, float* saved, const float* w_mf_host,
                                         const float* sumsq_partial, int32_t n_partial, float feat_reg_coef,
                                         float* scal4, double* running_sums3, llmrec_stream_t stream);
/* Clears exactly the rows llmrec_bpr_multi_bwd_f32 added into (dEu[u_b], dEi[p_b], dEi[q_b] of every problem, b < n_valid),
 * so scatter targets that start all-zero are all-zero again. */
int llmrec_bpr_multi_zero_rows_f32(int32_t n_problems, const llmrec_bpr_problem_t* problems_host, int32_t d,
                                   const int64_t* users, const int64_t* pos, const int64_t* neg,
                                   int32_t B_max, const int32_t* n_valid_dev, llmrec_stream_t stream);
/* The eight-problem loss segment of ONE LOCAL batch for B_max up to LLMREC_BPR_WIDE_MAX_B (additive: the entry points above keep
 * refusing B_max > LLMREC_BPR_MAX_B). Same `saved` / `plan` layouts; wherever both forms exist (B_max <= LLMREC_BPR_MAX_B) `plan`,
 * `saved`, `out`, `scal4`, the row flags and every gradient row carry the capped entry points' BITS. All hipGraph-capturable: the launch
 * sequence depends on the host arguments alone, integer atomics only, no host synchronisation, no allocation; every refusal is decided
 * before the first launch: a NULL or too-small workspace LLMREC_EWORKSPACE, B_max > LLMREC_BPR_WIDE_MAX_B LLMREC_EUNSUPPORTED (the
 * workspace queries: -1), a bad problem table or n_problems > LLMREC_BPR_MAX_PROBLEMS LLMREC_EINVAL.
 *   llmrec_bpr_scatter_plan_wide          llmrec_bpr_scatter_plan's LLMREC_BPR_PLAN_WORDS(B_max) words, word for word: the keys of both sides
 *                                         in one launch, one multi-block radix sort per side over the whole (distinct) keys - the sort of
 *                                         llmrec_scatter_rows_f32, between two buffers of the workspace -, then one launch that writes the
 *                                         sorted keys and the run lengths (an upper-bound binary search per run head). workspace:
 *                                         llmrec_bpr_scatter_plan_wide_workspace_bytes(B_max) bytes, 256-byte aligned.
 *   llmrec_bpr_multi_scores_wide_f32      llmrec_bpr_multi_scores_step_f32's launch (adamw_state3 == NULL: the row stamp only).
 *   llmrec_bpr_multi_select_bwd_wide_f32  llmrec_bpr_multi_select_bwd_f32 with llmrec_bpr_prune_fwd_wide_f32's exact radix select in place of
 *                                         rank counting in LDS: problem p owns block p of the workspace (histograms, state, eq[]), which
 *                                         the entry point's own launches initialise. Launches: init, four histogram passes, the ties'
 *                                         count, the write pass (coefficient -> saved[b], kept m_b or 0 -> slot 1, zeros for
 *                                         n_valid <= b < B_max, problem 0 stamps the rows; one more block per problem: the squared
 *                                         norms' sums and k into saved[B_max .. B_max + 3]), then the backward rows through `plan`.
 *                                         workspace: llmrec_bpr_multi_wide_workspace_bytes(n_problems, B_max) bytes, 4-byte aligned.
 *   llmrec_bpr_multi_losses_wide_f32      llmrec_bpr_multi_losses_assemble_f32's single-block launch; scal4 == NULL: the loss values only
 *                                         (out, saved[B_max .. B_max + 3]: llmrec_bpr_multi_losses_f32's bits), w_mf_host / sumsq_partial /
 *                                         running_sums3 are then not read.
 * Known limit: the backward gives one 16-lane group to each destination row, so at batches of 10^5 and more a popular item is one
 * long serial run of n_problems * (its count) rows - exact and deterministic, its time unmeasured. */
int64_t llmrec_bpr_scatter_plan_wide_workspace_bytes(int64_t B_max);
int llmrec_bpr_scatter_plan_wide(const int64_t* users, const int64_t* pos, const int64_t* neg, int32_t B_max, const int32_t* n_valid_dev,
                                 uint64_t* plan, void* workspace, int64_t workspace_bytes, llmrec_stream_t stream);
int llmrec_bpr_multi_scores_wide_f32(int32_t n_problems, const llmrec_bpr_problem_t* problems_host, int32_t d,
                                     const int64_t* users, const int64_t* pos, const int64_t* neg,
                                     int32_t B_max, const int32_t* n_valid_dev, float* saved, int32_t* row_stamp,
                                     float* adamw_state3, float lr, float beta1, float beta2, llmrec_stream_t stream);
int64_t llmrec_bpr_multi_wide_workspace_bytes(int32_t n_problems, int64_t B_max);
int llmrec_bpr_multi_select_bwd_wide_f32(int32_t n_problems, const llmrec_bpr_problem_t* problems_host, int32_t d,
                                         const int64_t* users, const int64_t* pos, const int64_t* neg,
                                         int32_t B_max, const int32_t* n_valid_dev, double remember_rate, float decay,
                                         float batch_size_flag, float* saved, uint8_t* user_row_flags, uint8_t* item_row_flags,
                                         const int32_t* row_stamp, const uint64_t* plan,
                                         void* workspace, int64_t workspace_bytes, llmrec_stream_t stream);
int llmrec_bpr_multi_losses_wide_f32(int32_t n_problems, int32_t B_max, const int32_t* n_valid_dev, double remember_rate, float decay,
                                     float batch_size_flag, float* out, float* saved, const float* w_mf_host,
                                     const float* sumsq_partial, int32_t n_partial, float feat_reg_coef,
                                     float* scal4, double* running_sums3, llmrec_stream_t stream);
/* dEu[u_b] += g_mf * ds_b * (Ei[p_b] - Ei[q_b]) + g_emb * c_u * Eu[u_b]   (deterministic scatter-add through `plan`, see above)
 * dEi[p_b] += g_mf * ds_b * Eu[u_b] + g_emb * c_p * Ei[p_b] ; dEi[q_b] likewise with -ds_b, c_q
 * g_mf / g_emb are upstream gradients read from device memory (grads2[0], grads2[1]). dEu and dEi are distinct buffers. */
int llmrec_bpr_prune_bwd_f32(const float* Eu, int64_t ldu, const float* Ei, int64_t ldi, int32_t d,
                             const int64_t* users, const int64_t* pos, const int64_t* neg,
                             int32_t B_max, const int32_t* n_valid_dev,
                             float decay, float batch_size_flag,
                             const float* saved, const float* grads2,
                             float* dEu, int64_t lddu, float* dEi, int64_t lddi, const uint64_t* plan, llmrec_stream_t stream);

/* The same gradient as COMPACT rows instead of a scatter (row-sharded step): rows3 = [3][B_max][d],
 * block 0 = d/dEu[u_b], block 1 = d/dEi[p_b], block 2 = d/dEi[q_b]; rows of samples b >= B are zero. The item rows are
 * what the ranks exchange (an all-gather of 2 B rows instead of an all-reduce of the dense I x d gradient). */
int llmrec_bpr_prune_bwd_rows_f32(const float* Eu, int64_t ldu, const float* Ei, int64_t ldi, int32_t d,
                                  const int64_t* users, const int64_t* pos, const int64_t* neg,
                                  int32_t B_max, const int32_t* n_valid_dev,
                                  float decay, float batch_size_flag,
                                  const float* saved, const float* grads2, float* rows3, llmrec_stream_t stream);

/* dst[ids[j]] += alpha * rows[j] for j < n, ids[j] < 0 skipped. Rows with the same id are added in ascending j
 * (radix sort of (id, j), one lane group per run): DETERMINISTIC, so ranks that scatter the same gathered rows keep
 * bit-identical replicas - a float-atomic scatter would not. */
int64_t llmrec_scatter_rows_workspace_bytes(int64_t n);
int llmrec_scatter_rows_f32(int64_t n, const int64_t* ids, const float* rows, int64_t ldr, int32_t d, float alpha,
                            float* dst, int64_t ldd, void* workspace, int64_t workspace_bytes, llmrec_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * R8  feature regulariser, optimiser     replaces (x**2).sum() x4 (reference main.py:151-156)
 *                                        and torch.optim.AdamW.step (main.py:100-104,278)
 * ------------------------------------------------------------------------------------------ */
/* out[0] (+)= coef * sum of squares of the rows x d block (deterministic two-level reduction) */
int64_t llmrec_sumsq_workspace_bytes(int64_t rows, int32_t d);
int llmrec_sumsq_f32(int64_t rows, int32_t d, const float* X, int64_t ldx, float coef, int32_t accumulate,
                     float* out, void* workspace, int64_t workspace_bytes, llmrec_stream_t stream);
/* Y (+)= alpha_dev[0] * alpha * X   (gradient of the regulariser; alpha_dev may be NULL = 1) */
int llmrec_axpy_f32(int64_t rows, int32_t d, float alpha, const float* alpha_dev, const float* X, int64_t ldx,
                    float* Y, int64_t ldy, int32_t accumulate, llmrec_stream_t stream);

/* out_g[j] (+)= sum_r w[r] * X[r][group_width g + j] for the n_groups column groups of X (w NULL = ones); groups that name the same
 * destination are summed in group order; two-level, fixed order (deterministic). The bias gradient of projections whose operand was
 * propagated beforehand (llmrec_linear_problem_t.bias_scale): db = sum_r bias_scale[r] dY[r]; one call serves every Linear of the
 * [rows, 7 d] gradient buffer (reference: the autograd bias gradients of Models.py:145-150). group_width <= 64, n_groups <= MAX_GROUPS. */
#define LLMREC_COLSUM_MAX_GROUPS 8
int64_t llmrec_weighted_colsum_workspace_bytes(int32_t n_columns);
int llmrec_weighted_colsum_f32(int64_t rows, int32_t n_groups, int32_t group_width, const float* X, int64_t ldx, const float* w,
                               float* const* group_out_host, int32_t accumulate,
                               void* workspace, int64_t workspace_bytes, llmrec_stream_t stream);

/* Clear up to LLMREC_ZERO_MAX_TENSORS fp32 buffers in ONE launch (the backward's scatter targets; replaces
 * one aten::zero_ per tensor inside the captured step). */
#define LLMREC_ZERO_MAX_TENSORS 8
typedef struct { float* p; int64_t n; } llmrec_zero_tensor_t;
int llmrec_zero_multi_f32(int32_t n_tensors, const llmrec_zero_tensor_t* tensors_host, llmrec_stream_t stream);
/* dst[ids[j]][0..d) = 0 for j < n (ids[j] < 0 skipped): row-wise clean-up of a scatter target whose other rows are already zero
 * (the row-sharded step scatters B gradient rows into 10^7-row tables; replaces a dense aten::zero_ per step) */
int llmrec_zero_rows_f32(int64_t n, const int64_t* ids, int32_t d, float* dst, int64_t ldd, llmrec_stream_t stream);

/* Loss assembly of reference main.py:273 / :280-283 on the device, one single-wave launch (replaces the
 * aten mul / sum / add / copy launches that assembled the logged scalars):
 *   bpr_out [n_problems][2] = (mf, emb) of each BPR problem; w_mf_host[n_problems] = its weight in the loss;
 *   scal[4] = [feat_reg (input), loss, mf, emb].
 *   mode 0 (single GPU): scal[1] = sum_p w_mf[p] * mf_p + emb_0 + scal[0]; scal[2] = mf_0; scal[3] = emb_0
 *   mode 1 (batch-sharded replica, before the gradient all-reduce): tail[p] = mf_p (this rank's share),
 *          tail[n_problems] = (emb_0 + scal[0]) * inv_world
 *   mode 2 (after it): scal[2] = tail[0]; scal[3] = emb_0; scal[1] = sum_p w_mf[p] * tail[p] + tail[n_problems]
 *   running_sums3 (optional, modes 0 and 2): running_sums3[0..2] += (loss, mf, emb) in double - the epoch sums of the reference's log line
 *   (main.py:280-283) accumulated inside the step graph, so a loop of graph replays needs no host-side arithmetic per step */
int llmrec_loss_assemble_f32(int32_t mode, int32_t n_problems, const float* bpr_out, const float* w_mf_host,
                             float* scal4, float* tail, float inv_world, double* running_sums3, llmrec_stream_t stream);

/* out[b] = scale * sum_t terms[t][idx[b]] for b < n: the layer mean of reference Models.py:185-186 for the rows a batch
 * needs only (row-sharded step: B rows instead of a pass over the 10^7-row user tables) */
int llmrec_gather_mean_f32(int64_t n, const int64_t* idx, int32_t d, float scale, int32_t n_terms,
                           const float* const* terms, const int64_t* term_ld, float* out, int64_t ldo, llmrec_stream_t stream);
/* Y[r] = s[r] * X[r] (Y may alias X) */
int llmrec_scale_rows_f32(int64_t rows, int32_t d, const float* s, const float* X, int64_t ldx, float* Y, int64_t ldy,
                          llmrec_stream_t stream);

/* state[0] = step count (as float bits of an int32), state[1] = lr / (1 - b1^t), state[2] = sqrt(1 - b2^t).
 * llmrec_adamw_advance increments t on the device and refreshes state[1..2]. */
int llmrec_adamw_advance(float* state3, float lr, float beta1, float beta2, llmrec_stream_t stream);
/* decoupled weight decay, then Adam (torch.optim.AdamW, amsgrad=False, maximize=False) */
int llmrec_adamw_f32(int64_t n, float* p, const float* g, float* m, float* v, const float* state3,
                     float lr, float beta1, float beta2, float eps, float weight_decay, llmrec_stream_t stream);

/* the same update for up to LLMREC_ADAMW_MAX_TENSORS parameters in one launch: one block per LLMREC_ADAMW_CHUNK elements of a tensor. A
 * chunk that lies inside its tensor and whose p / g / m / v / g_out are 16-byte aligned moves as float4 (every load of a thread issued
 * before its first arithmetic); a tensor's tail chunk and misaligned views take 4-byte accesses. Both call one per-element update: the
 * bits are those of llmrec_adamw_f32 either way. */
#define LLMREC_ADAMW_MAX_TENSORS 16
#define LLMREC_ADAMW_CHUNK 1024
typedef struct { float* p; const float* g; float* m; float* v; int64_t n;
                 float g_scale;   /* the gradient is g_scale * g (non-zero; 1 = plain): saves a scaling pass over a large table */
                 float* g_out;    /* optional: receives the gradient the update used (g_scale * g) - the parameter's .grad when g is another
                                     buffer (the user table's gradient IS inv * dE_u: no separate axpy launch); NULL = not stored */
} llmrec_adamw_tensor_t;
int llmrec_adamw_multi_f32(int32_t n_tensors, const llmrec_adamw_tensor_t* tensors_host, const float* state3,
                           float lr, float beta1, float beta2, float eps, float weight_decay, llmrec_stream_t stream);
/* The same update and, in the same launch (extra blocks), the row-wise clean-up of scatter targets: for every job j < n_jobs and every
 * b < min(*n_valid_dev, B_cap): dst_j[ids_j[b], 0 .. d_j) = 0 (what llmrec_bpr_multi_zero_rows_f32 does with its own launch; a job may span
 * the adjacent column slices several problems scattered into). The caller orders the launch behind the last reader of those rows. */
#define LLMREC_ZERO_ROWS_MAX_JOBS 24
typedef struct { const int64_t* ids; float* dst; int64_t ldd; int32_t d; } llmrec_zero_rows_job_t;
int llmrec_adamw_multi_zero_rows_f32(int32_t n_tensors, const llmrec_adamw_tensor_t* tensors_host, const float* state3,
                                     float lr, float beta1, float beta2, float eps, float weight_decay,
                                     int32_t n_jobs, const llmrec_zero_rows_job_t* jobs_host, int32_t B_cap, const int32_t* n_valid_dev,
                                     llmrec_stream_t stream);

/* The three independent row sweeps a one-stream training step issues right behind its loss backward, as ONE launch of three block
 * ranges: llmrec_fuse_bwd_src_multi_f32 (n_fuse_problems, fuse_host, d), llmrec_adamw_multi_f32 (n_tensors ... weight_decay) and
 * llmrec_softmax_rows_bwd_scaled_f32 (sm_rows, sm_d, sm_alpha ... sm_lddz), each with the argument checks and, bit for bit, the result
 * of its own entry point (the kernels share the row / chunk bodies). A member is absent when its count is 0 (n_fuse_problems = 0,
 * n_tensors = 0, sm_rows = 0). The caller guarantees that no member writes what another reads. Only the instance the step runs is
 * compiled - 16-byte accesses and d, sm_d <= 64; for anything else the call returns LLMREC_EUNSUPPORTED WITHOUT launching and the caller
 * issues the three launches itself. */
int llmrec_step_rows_group_f32(int32_t n_fuse_problems, const llmrec_fuse_bwd_problem_t* fuse_host, int32_t d,
                               int32_t n_tensors, const llmrec_adamw_tensor_t* tensors_host, const float* state3,
                               float lr, float beta1, float beta2, float eps, float weight_decay,
                               int64_t sm_rows, int32_t sm_d, float sm_alpha, const float* sm_Y, int64_t sm_ldy, const float* sm_dY, int64_t sm_lddy,
                               float* sm_dZ, int64_t sm_lddz, llmrec_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * R9/R10  full-rank scoring + masked top-K + hit vectors
 *                                        replaces torch.matmul(E_u[blk], E_i^T), the D2H copy of
 *                                        the 2048 x I score block and the per-user Python
 *                                        set-difference + heapq.nlargest
 *                                        (reference utility/batch_test.py:21-36,83-109,149-157)
 * For each listed user: scores over all items (fp32 MFMA), train items removed (CSR row of the
 * user, ascending columns), top K by (score desc, item id asc). The U x I matrix is never
 * written. Missing entries (fewer than K candidates) are -1 / -inf.
 * K <= LLMREC_TOPK_MAX for the single-sweep calls (llmrec_score_topk_f32 / _ws_f32 / _mode_f32: every
 * selection structure of the sweeps is a 64-slot list, one slot per lane); llmrec_score_topk_wide_f32
 * (below) ranks up to LLMREC_TOPK_WIDE_MAX items per user by repeating the sweep over a growing mask.
 * Tables: 1 <= d <= 128 (d > 128: LLMREC_EUNSUPPORTED, refused before anything is launched or
 * written), any ld >= d, any 4-byte-aligned base - a column view of a wider table is fine.
 * The sweeps' vector path (16-byte loads of the rows) needs ldu % 4 == 0, ldi % 4 == 0 and both
 * bases 16-byte aligned, and the unguarded instances also d % 16 == 0; every other table goes
 * through guarded loads that read nothing outside [row, row + d): the same bits (their speed
 * is not measured). llmrec_score_auc_f32 alone needs d % 16 == 0.
 * ------------------------------------------------------------------------------------------ */
#define LLMREC_TOPK_MAX 64
int llmrec_score_topk_f32(int32_t n_query, const int64_t* query_users,
                          const float* Eu, int64_t ldu, const float* Ei, int64_t ldi,
                          int64_t n_items, int32_t d,
                          const int32_t* train_rowptr, const int32_t* train_colidx,
                          int32_t K, int32_t* out_idx /* n_query x K */, float* out_score /* n_query x K */,
                          llmrec_stream_t stream);
/* The same with a workspace of llmrec_score_topk_workspace_bytes(n_query, n_items, d) bytes (16-byte aligned):
 *   - the item table is first re-laid in MFMA fragment order (one pass over Ei, written into the workspace), so that every load of
 *     the sweep is one contiguous KB instead of 64 row pieces;
 *   - the user tiles left over after the last full round of one 16-user tile per compute unit are each swept by several
 *     blocks (parts of the item range) whose 64-slot lists are merged by a second launch, spreading the left-over blocks over the device;
 *   - with a train CSR and at most 131 072 items: a block turns the rows of up to two of its users with more than 48 train items into
 *     bitmaps (one word per 32-item tile, in its own slice of the workspace) and reads one word per round instead of walking the row.
 * The lists and scores are the same, bit for bit. workspace == NULL behaves like llmrec_score_topk_f32. */
/* Tuning knob of the bf16 sweep's ITEM PARTS (tables beyond the L2: every user tile is cut into parts of `items` items whose fragments fit an
 * XCD's L2, block ids part-major; csrc/topk.hip plan_parts): 0 = the library's policy (8 MB of fragments per part for tables beyond 131 072 items),
 * -1 = never, else a multiple of 32 >= 1024. Process-wide; set it BEFORE sizing a workspace (llmrec_score_topk_workspace_bytes depends on it). */
int llmrec_topk_set_part_items(int32_t items);
int64_t llmrec_score_topk_workspace_bytes(int32_t n_query, int64_t n_items, int32_t d);
int llmrec_score_topk_ws_f32(int32_t n_query, const int64_t* query_users,
                             const float* Eu, int64_t ldu, const float* Ei, int64_t ldi,
                             int64_t n_items, int32_t d,
                             const int32_t* train_rowptr, const int32_t* train_colidx,
                             int32_t K, int32_t* out_idx /* n_query x K */, float* out_score /* n_query x K */,
                             void* workspace, int64_t workspace_bytes, llmrec_stream_t stream);
/* debug / test entry: the full score block with the same MFMA arithmetic as above */
/* The same call with the sweep's arithmetic chosen explicitly (round 5). Lists and scores are BIT-IDENTICAL in both modes:
 *   LLMREC_TOPK_MODE_EXACT_SWEEP  every score by the exact-fp32 MFMA chain (what llmrec_score_topk_ws_f32 runs);
 *   LLMREC_TOPK_MODE_PREFILTER    the sweep on bf16 MFMAs (both operands as two round-to-nearest bf16 terms, three products:
 *                                 |s - s'| <= c ||u|| ||i||, c = 2^-14 for d <= 64 and 2^-13 above) keeps each user's 64 best items by the
 *                                 UPPER BOUND ub = s' + c ||u|| ||i||;
 *                                 those 64 are then scored with the exact fp32 fma chain, re-ranked, and VERIFIED: (64th ub) < (K-th exact
 *                                 score) proves that no other item can be in the top K. User tiles that fail the proof are swept again by the
 *                                 exact kernel (second launch; the other tiles' blocks exit at once).
 *                                 MAGNITUDES: the guarantee holds for every finite table. The bound's own fp32 arithmetic is trusted for rows
 *                                 with 2^-44 <= ||x|| <= 2^44 and for all-zero rows; an item row outside that window has the bound +inf
 *                                 (always kept and scored exactly), a user row outside it sends its tile to the exact sweep. Tables whose
 *                                 scores are normal fp32 numbers get the exact sweep's bits in both modes at any scale; only the
 *                                 mode's speed belongs to the window. Needs the workspace;
 *                                 K <= LLMREC_TOPK_PREFILTER_MAX_K (else the exact sweep runs). llmrec_score_topk_stats_offset: byte offset inside
 *                                 the workspace of three uint32 words the mode leaves behind - [0] = the drains of the sweep's candidate
 *                                 pools, summed over its blocks (round 6), [1] = the number of user tiles the exact sweep had to redo, [2] = the
 *                                 number of train rows the blocks swept as bitmaps (long rows; all 16 rows of a user tile with dense rows). */
#define LLMREC_TOPK_PREFILTER_MAX_K 56
#define LLMREC_TOPK_MODE_EXACT_SWEEP 0
#define LLMREC_TOPK_MODE_PREFILTER 1
int llmrec_score_topk_mode_f32(int32_t n_query, const int64_t* query_users,
                               const float* Eu, int64_t ldu, const float* Ei, int64_t ldi,
                               int64_t n_items, int32_t d,
                               const int32_t* train_rowptr, const int32_t* train_colidx,
                               int32_t K, int32_t* out_idx, float* out_score,
                               void* workspace, int64_t workspace_bytes, int32_t mode, llmrec_stream_t stream);
int64_t llmrec_score_topk_stats_offset(int32_t n_query, int64_t n_items);
/* Cut-offs beyond the 64 slots of a sweep: the same ranking rule (exact-fp32 scores - the bits of llmrec_scores_f32 -, train items removed,
 * (score desc, item id asc), missing entries -1 / -inf, out_idx / out_score [n_query][K]) for K <= LLMREC_TOPK_WIDE_MAX.
 *   K <= LLMREC_TOPK_MAX: forwards to llmrec_score_topk_mode_f32 (same launches, same bits; train_nnz is not read).
 *   K >  LLMREC_TOPK_MAX: ROUNDS. The order is a strict total order, so ranks [c p, c (p + 1)) of a user are the top c of (candidates minus
 *     the user's first c p items): the masked top-K call runs ceil(K / c) times, c = LLMREC_TOPK_PREFILTER_MAX_K in the prefilter mode and
 *     LLMREC_TOPK_MAX in the exact mode (the last pass asks for the K - c p items still missing), each time with the items already emitted
 *     joined to the mask. Every pass is an ordinary llmrec_score_topk_mode_f32 call over a compact copy of the queried user rows (identity
 *     query list, the same score bits) and a mask CSR of n_query + 1 row pointers that the pass rebuilds on the device: row q = the ascending
 *     merge of query q's train row (duplicates kept) with the ids emitted for q so far (entries < 0 are never merged). So the first 64
 *     columns equal the K = 64 answer of the single-sweep call bit for bit, duplicate or unsorted query users are fine, and a pass costs one
 *     call at K = c plus three small launches (row pointers: one single-block scan; rows: one wave per query; the strided write of the pass's
 *     columns into the outputs). 1 + passes x (3 + the launches of the call) launches, a function of the host arguments alone; capturable,
 *     deterministic (no atomics), no allocation.
 *   train_nnz: the capacity reserved for train entries in the rebuilt mask - at least the sum of the train-row lengths of the query users,
 *     a user listed twice counted twice (the CSR's entry count when the query users are distinct; 0 without a train CSR). A smaller value
 *     is a caller error that the device detects before anything is written: every list then comes back empty (-1 / -inf).
 *     train_nnz + n_query * K must stay below 2^31.
 *   Workspace (required for K > LLMREC_TOPK_MAX, 16-byte aligned; too small: LLMREC_EWORKSPACE). With A(x) = x rounded up to 256:
 *     llmrec_score_topk_wide_workspace_bytes = llmrec_score_topk_workspace_bytes(n_query, n_items, d)                       for K <= 64, else that
 *       + A(4 n_query d4) + A(8 n_query) + 2 A(4 (n_query + 1)) + A(4 n_query) + 256 + 2 A(4 (train_nnz + n_query K)) + 2 A(4 * 64 n_query)
 *     (d4 = d rounded up to 4: the user rows; the query list; two generations of row pointers; the per-query counts of the last pass; the
 *     overflow word; two generations of mask columns; the ids and scores of one pass). -1 for bad sizes (K outside 1 .. 1024 included). */
#define LLMREC_TOPK_WIDE_MAX 1024
int64_t llmrec_score_topk_wide_workspace_bytes(int32_t n_query, int64_t n_items, int32_t d, int32_t K, int64_t train_nnz);
int llmrec_score_topk_wide_f32(int32_t n_query, const int64_t* query_users,
                               const float* Eu, int64_t ldu, const float* Ei, int64_t ldi,
                               int64_t n_items, int32_t d,
                               const int32_t* train_rowptr, const int32_t* train_colidx,
                               int32_t K, int32_t* out_idx, float* out_score,
                               void* workspace, int64_t workspace_bytes, int32_t mode, int64_t train_nnz, llmrec_stream_t stream);
int llmrec_scores_f32(int32_t n_query, const int64_t* query_users,
                      const float* Eu, int64_t ldu, const float* Ei, int64_t ldi,
                      int64_t n_items, int32_t d, float* S, int64_t lds, llmrec_stream_t stream);
/* hits[q, j] = 1 if topk_idx[q, j] is in the held-out CSR row of query_users[q]
 * (reference batch_test.py:29-34) */
int llmrec_topk_hits(int32_t n_query, const int64_t* query_users, int32_t K, const int32_t* topk_idx,
                     const int32_t* test_rowptr, const int32_t* test_colidx, uint8_t* hits,
                     llmrec_stream_t stream);
/* R10 (reference utility/metrics.py:8-18,43-87 through batch_test.py:70-80): per-user precision, recall, ndcg and
 * hit-ratio at each of the n_ks <= 8 cut-offs (host array ks), in double, from the hit matrix of llmrec_topk_hits and
 * the ranked lists: out[q][4][n_ks]. ndcg uses the reference's IDCG (the retrieved hit vector sorted descending);
 * precision averages over the ranked items that exist. The caller sums over users (12 doubles leave the device
 * instead of n x K hits). */
int llmrec_topk_metrics(int32_t n_query, const int64_t* query_users, int32_t K, const uint8_t* hits, const int32_t* topk_idx,
                        const int32_t* test_rowptr, int32_t n_ks, const int32_t* ks_host, double* out, llmrec_stream_t stream);
/* Round 6 - a whole evaluation's R10 in two launches (what batch_test.py:160-165 accumulates over the users): out[4][n_ks] = the SUMS over the
 * query users of precision, recall, ndcg, hit-ratio at every cut-off (the caller divides by the number of users), from the ranked lists and the
 * held-out CSR directly - the hit flags and the per-user values stay in registers, the users are added by fixed trees (deterministic). K <= LLMREC_TOPK_WIDE_MAX:
 * up to K = 128 one thread per user with the hit flags in two 64-bit words; beyond (csrc/topk_wide.hip) one wave per user, a lane-private bit
 * per rank, the sums over ranks by lane and butterfly (the same values up to the order of the double additions). Same workspace either way.
 * `out` may be device memory or mapped (pinned) host memory: an evaluation graph then ends with the twelve doubles already on the host. */
int64_t llmrec_topk_eval_sums_workspace_bytes(int32_t n_query, int32_t n_ks);
int llmrec_topk_eval_sums(int32_t n_query, const int64_t* query_users, int32_t K, const int32_t* topk_idx, const int32_t* test_rowptr,
                          const int32_t* test_colidx, int32_t n_ks, const int32_t* ks_host, void* workspace, int64_t workspace_bytes,
                          double* out, llmrec_stream_t stream);
/* Full-rank AUC (reference utility/batch_test.py:38-68,104-108, --test_flag full) without a score leaving the device. For each query
 * user u:  T = u's train row;  H = u's held-out row (val or test, as for llmrec_topk_eval_sums) taken as a SET - duplicates and ids outside
 * [0, n_items) do not count;  C = [0, n_items) \ T the candidates;  P = H & C the positives;  N = C \ H the negatives;  s_i = the score
 * BITS llmrec_scores_f32 gives (u, i) (the exact-fp32 chain the top-K sweep ranks by). Then
 *     c2_u  = sum over p in P, n in N of (2 [s_p > s_n] + [s_p == s_n])          (integer; float equality: +0.0 == -0.0 is a tie)
 *     AUC_u = c2_u / (2 |P| |N|)                                                 (double)
 *     AUC_u = 0 if |P| == 0 or |N| == 0, or if some s_i with i in C is NaN or +-inf (then c2_u is reported as 0)
 * - what sklearn's roc_auc_score gives over the candidates, and 0 where it raises (utility/metrics.py auc).
 * Rows of both CSRs ascending (llmrec_csr_build); train may be null (nothing masked). d a multiple of 16, at most 128 (LLMREC_EINVAL otherwise);
 * ld and base as for the top-K calls above.
 * Outputs, each optional: auc_out[n_query] (double), counts_out[n_query][3] = (c2, |P|, |N|) (int64), sum_out[1] = the sum of the
 * per-user AUCs by a fixed tree (device memory or mapped pinned host memory, as for llmrec_topk_eval_sums; the caller divides by n_query).
 * Integer counts and fixed-order sums: the results are deterministic. Four launches, capturable; no allocation. */
int64_t llmrec_score_auc_workspace_bytes(int32_t n_query, int64_t n_items, int32_t d);
int llmrec_score_auc_f32(int32_t n_query, const int64_t* query_users,
                         const float* Eu, int64_t ldu, const float* Ei, int64_t ldi,
                         int64_t n_items, int32_t d,
                         const int32_t* train_rowptr, const int32_t* train_colidx,
                         const int32_t* held_rowptr, const int32_t* held_colidx,
                         double* auc_out, int64_t* counts_out, double* sum_out,
                         void* workspace, int64_t workspace_bytes, llmrec_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Serving: exact masked top-K under an item ALLOW-LIST (csrc/serve.hip: the filter build and the pipeline of both scoring entries). No counterpart in the reference, which ranks the whole
 * catalogue for its test users only (utility/batch_test.py). Additive: the ABI version stays.
 * For query user u, an allow mask allow[0 .. n_items) (uint8, ANY non-zero byte = eligible) and an optional train CSR the candidates are
 *     { i : allow[i] != 0 and i not in the train row of u };
 * the result is the first K of them by (score desc, ORIGINAL item id asc), the scores the bits llmrec_scores_f32 gives, entries behind the
 * last candidate -1 / -inf: the rule and the arithmetic of llmrec_score_topk_wide_f32. The filter is applied by COMPACTION: the eligible
 * rows of Ei become a dense table, the queried train rows are rewritten in its numbering, the wide call runs on that table and the ids
 * are mapped back. A score is a per-pair fma chain that does not depend on where a row sits, and the compact numbering is monotone in
 * the item id, so order and bits are those of a sweep over the whole table - and a filter that keeps a tenth of the catalogue sweeps a
 * tenth of it.
 *
 * llmrec_item_filter_build: new_id[i] = the rank of i among the eligible items or -1, old_id[r] = the r-th eligible item (entries at and
 *   beyond the count are not written), n_kept_dev[0] = their count. An exclusive scan of the flags over blocks of LLMREC_FILTER_TILE
 *   items in three launches - per-block counts, one block scanning the counts, the write -, every cross-block hand-over a kernel boundary:
 *   no block waits for another, no atomics; deterministic, capturable, nothing read back. n_items in [0, 2^31).
 *   Workspace: llmrec_item_filter_workspace_bytes = A(4 ceil(n_items / LLMREC_FILTER_TILE)) + 256, A(x) = x rounded up to 256.
 *
 * llmrec_score_topk_filtered_f32: the arguments of llmrec_score_topk_wide_f32 (same meaning; 1 <= d <= 128, any ld >= d; query users may
 *   be unsorted and repeated; mode as there) + the maps of the build + the HOST integer n_kept, which sizes the compact table and the
 *   launches (the caller reads it once per filter). n_kept == 0: the outputs are filled with -1 / -inf and no sweep is launched (the
 *   sweeps refuse an empty table). Otherwise, on the caller's one stream:
 *     (a) the compact item table [n_kept][d4] through old_id (d4 = d rounded up to 4, pad columns zero, 256-byte aligned base - the sweeps'
 *         vector path applies; row offsets old * ldi in 64 bits);
 *     (b) the compact user rows [n_query][d4] + the identity query list;
 *     (c) the mask CSR, n_query + 1 row pointers: row q = the entries c of the train row of query_users[q] with new_id[c] >= 0, written
 *         as new_id[c] in row order (ascending stays ascending; duplicates are kept, as llmrec_csr_build keeps them) - count per query,
 *         one single-block scan, write;
 *     (d) llmrec_score_topk_wide_f32 on the compact tables with the mask as its train CSR (no train CSR: none);
 *     (e) the ids through old_id; -1 stays -1.
 *   6 launches (3 without a train CSR) + those of the wide call, a function of the host arguments alone; no allocation, no host read, no
 *   atomics: capturable and deterministic.
 *   train_nnz: the capacity of (c) and of the wide call - an upper bound of the sum of the queried train-row lengths, a user listed twice
 *     counted twice (not read without a train CSR). train_nnz + n_query * K must stay below 2^31 for K > LLMREC_TOPK_MAX.
 *   Caller errors the DEVICE detects before anything is written outside a buffer - every list then comes back empty (-1 / -inf) and the
 *     call returns LLMREC_OK, as the wide call does for a short train_nnz: n_kept != n_kept_dev[0] (the compact table is then zero-filled:
 *     (a) reads old_id only at ranks < n_kept and only when the counts agree), and a mask that outgrows train_nnz (its row pointers are
 *     then all zero and no column is written).
 *   Workspace (16-byte aligned; too small: LLMREC_EWORKSPACE): llmrec_score_topk_filtered_workspace_bytes = 0 for n_kept == 0, else
 *       A(llmrec_score_topk_wide_workspace_bytes(n_query, n_kept, d, K, train_nnz))
 *       + A(4 n_kept d4) + A(4 n_query d4) + A(8 n_query) + 256 + A(4 n_query) + A(4 (n_query + 1)) + A(4 train_nnz) + 256
 *     (the wide call's workspace; item rows; user rows; query list; error word; per-query counts; mask row pointers; mask columns), -1
 *     for bad sizes. llmrec_score_topk_filtered_mask_offset: the byte offset of the mask row pointers inside that workspace (the
 *     columns follow at + A(4 (n_query + 1))): what a test reads (c) from; -1 where there is no mask (bad sizes, n_kept == 0).
 * ------------------------------------------------------------------------------------------ */
#define LLMREC_FILTER_TILE 2048
int64_t llmrec_item_filter_workspace_bytes(int64_t n_items);
int llmrec_item_filter_build(int64_t n_items, const uint8_t* allow, int32_t* new_id /* n_items */, int32_t* old_id /* n_items */,
                             int32_t* n_kept_dev /* 1 */, void* workspace, int64_t workspace_bytes, llmrec_stream_t stream);
int64_t llmrec_score_topk_filtered_workspace_bytes(int32_t n_query, int64_t n_items, int32_t n_kept, int32_t d, int32_t K, int64_t train_nnz);
int64_t llmrec_score_topk_filtered_mask_offset(int32_t n_query, int64_t n_items, int32_t n_kept, int32_t d, int32_t K, int64_t train_nnz);
int llmrec_score_topk_filtered_f32(int32_t n_query, const int64_t* query_users,
                                   const float* Eu, int64_t ldu, const float* Ei, int64_t ldi,
                                   int64_t n_items, int32_t d,
                                   const int32_t* train_rowptr, const int32_t* train_colidx,
                                   int32_t K, int32_t* out_idx, float* out_score,
                                   void* workspace, int64_t workspace_bytes, int32_t mode, int64_t train_nnz,
                                   const int32_t* new_id, const int32_t* old_id, const int32_t* n_kept_dev, int32_t n_kept,
                                   llmrec_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Serving with PER-QUERY exclusion lists (the pipeline of csrc/serve.hip with the exclusion stage of csrc/exclude.hip): items a user bought, saw or dismissed since the graph was built, items
 * already shown, the earlier pages of a result. Additive: the ABI version stays, and llmrec_score_topk_filtered_f32 is unchanged.
 *
 * llmrec_score_topk_excluded_f32: the arguments of llmrec_score_topk_wide_f32 up to train_nnz (same meaning; 1 <= d <= 128; query users may
 *   be unsorted and repeated), an exclusion CSR over the QUERIES of this call, and the filter arguments of the filtered call.
 *   Result: for every query q the first K items of
 *       { eligible items } minus { train row of query_users[q] } minus { exclusion row q }
 *   by (score desc, ORIGINAL item id asc), the scores the bits of llmrec_scores_f32, -1 / -inf behind the last candidate, ids ORIGINAL ids.
 *   The exclusion CSR: excl_rowptr [n_query + 1], excl_colidx [excl_nnz], int32, on the device. Row q belongs to QUERY q, not to a user:
 *     a user listed twice may carry two different rows. Entries come in any order and may repeat. An entry < 0 or >= n_items is ignored
 *     (-1 padding, as a previous call's output has it); with a filter so is an entry whose item is ineligible.
 *     excl_rowptr == NULL with excl_nnz == 0: no exclusions (excl_colidx is then not read). excl_nnz is the EXACT entry count,
 *     excl_rowptr[n_query]; excl_nnz > 0 needs both pointers.
 *   The filter: new_id / old_id / n_kept_dev all NULL with n_kept == n_items: NO FILTER - the numbering is the identity, Ei is swept in
 *     place through ldi (no item gather, no copy of the table) and no id is mapped back. Otherwise the three maps of
 *     llmrec_item_filter_build and the host's n_kept, with the hand-shake of the filtered call (n_kept != n_kept_dev[0] sets the error
 *     word). Maps that keep every item (n_kept == n_items) number the items as they are: Ei is swept in place then too.
 *   The mask the sweeps read, n_query + 1 row pointers: row q = the ascending STABLE merge of
 *       the train row's kept entries in the swept numbering, in row order - exactly row q of the filtered call's mask -, and
 *       the exclusion row's kept entries in the swept numbering, sorted ascending;
 *     duplicates are kept on both sides, and a train entry comes before an equal exclusion entry.
 *   On the caller's one stream: (a) the compact user rows + the identity query list, and with a filter the compact item table, as the
 *     filtered call; (b) entry e of exclusion row q (q by binary search in excl_rowptr) -> the 64-bit key q << 32 | id, a dropped entry ->
 *     n_query << 32, behind every row; the same launch checks excl_rowptr; (c) one radix sort of the keys (the vendor sort of
 *     llmrec_scatter_rows_f32, between two buffers of the workspace, bits [0, 32 + bits of n_query)); (d) per query the kept train count and
 *     the lower bound of q << 32 in the sorted keys - the bound IS the exclusive scan of the kept exclusion counts; (e) one single-block scan:
 *     the row pointers of the train side and, + the bounds, of the merged mask; (f) the train side's rows; (g) the merge, one wave per query,
 *     wave-strided: a train entry lands at its index + the number of the query's keys below it, a key at its index + the number of train
 *     entries at or below it, both by binary search - rows of thousands of entries need no LDS; (h) llmrec_score_topk_wide_f32 over the
 *     swept tables with the merged mask, capacity train_nnz + excl_nnz; (i) ids through old_id (filter only) and, under the error word, -1 / -inf.
 *     6 launches (5 without an exclusion CSR) + 1 with a filter + 1 with a train CSR + the sort's + the wide call's: a function of the host
 *     arguments alone; no allocation, no host read, no atomics, every cross-block hand-over a kernel boundary: capturable and deterministic.
 *   train_nnz: as for the filtered call (an upper bound of the sum of the queried train-row lengths; not read without a train CSR).
 *     train_nnz + excl_nnz + n_query * K must stay below 2^31 (at every K).
 *   Caller errors the DEVICE detects before anything is written outside a buffer - every list then comes back empty (-1 / -inf) and the call
 *     returns LLMREC_OK: a train side that outgrows train_nnz; an excl_rowptr that does not start at 0, end at excl_nnz and never decrease;
 *     n_kept != n_kept_dev[0]. The mask's row pointers are then all zero and no column is written.
 *   n_kept == 0: the outputs are filled with -1 / -inf and no sweep is launched. n_query == 0: no launch.
 *   Workspace (16-byte aligned; too small: LLMREC_EWORKSPACE): llmrec_score_topk_excluded_workspace_bytes = 0 for n_kept == 0, else
 *       A(llmrec_score_topk_wide_workspace_bytes(n_query, n_kept, d, K, train_nnz + excl_nnz))
 *       + [n_kept != n_items: A(4 n_kept d4)] + A(4 n_query d4) + A(8 n_query) + 256 + A(4 n_query) + 2 A(4 (n_query + 1))
 *       + A(4 train_nnz) + 256 + 2 A(8 excl_nnz) + [excl_nnz > 0: A(excl_nnz + 32 MiB)]
 *       + A(4 (n_query + 1)) + A(4 (train_nnz + excl_nnz)) + 256
 *     (the wide call's workspace; item rows; user rows; query list; error word; train counts; train row pointers and key bounds; train
 *     columns; two key buffers; the sort's temporary storage, the bound of llmrec_scatter_rows_workspace_bytes - a sort that asks for more
 *     is LLMREC_EWORKSPACE before the first launch; mask row pointers; mask columns), -1 for bad sizes, the 2^31 sum included.
 *     llmrec_score_topk_excluded_mask_offset: the byte offset of the merged mask's row pointers inside that workspace (the columns follow at
 *     + A(4 (n_query + 1)), as the filtered call lays them out); -1 where there is no mask (bad sizes, n_kept == 0).
 * ------------------------------------------------------------------------------------------ */
int64_t llmrec_score_topk_excluded_workspace_bytes(int32_t n_query, int64_t n_items, int32_t n_kept, int32_t d, int32_t K, int64_t train_nnz,
                                                   int64_t excl_nnz);
int64_t llmrec_score_topk_excluded_mask_offset(int32_t n_query, int64_t n_items, int32_t n_kept, int32_t d, int32_t K, int64_t train_nnz,
                                               int64_t excl_nnz);
int llmrec_score_topk_excluded_f32(int32_t n_query, const int64_t* query_users,
                                   const float* Eu, int64_t ldu, const float* Ei, int64_t ldi,
                                   int64_t n_items, int32_t d,
                                   const int32_t* train_rowptr, const int32_t* train_colidx,
                                   int32_t K, int32_t* out_idx, float* out_score,
                                   void* workspace, int64_t workspace_bytes, int32_t mode, int64_t train_nnz,
                                   const int32_t* excl_rowptr /* n_query + 1 */, const int32_t* excl_colidx, int64_t excl_nnz,
                                   const int32_t* new_id, const int32_t* old_id, const int32_t* n_kept_dev, int32_t n_kept,
                                   llmrec_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Serving with PER-QUERY candidate lists (csrc/candidates.hip): "here are this request's candidates; rank them for this user" - the output
 * of a retrieval stage, a campaign's items, a shop's shelf. Only the listed pairs are scored; the sweeps are not involved. Additive: the
 * ABI version stays, and no other prototype changes.
 *
 * llmrec_score_topk_candidates_f32: query users (unsorted, repeats allowed), the two tables (1 <= d <= 128, any ld >= d, any 4-byte-aligned
 *   base: nothing outside [row, row + d) is read on any layout), the train CSR or NULL, K >= 1 with n_query * K < 2^31 (NO 1024 cap: nothing
 *   here is sized by K except the final write), a candidate CSR and an optional exclusion CSR over the QUERIES of this call, and new_id of
 *   an item filter or NULL (only new_id is read; nothing is compacted and no id is mapped back).
 *   Result: for query q with user u = query_users[q], the ids of candidate row q taken as a SET (repeats collapse; an id < 0, >= n_items
 *   or with new_id[id] < 0 is ignored) minus { train row of u } minus { exclusion row q }; the first K of what remains by
 *   (score desc, ORIGINAL item id asc), the scores the bits of llmrec_scores_f32, -1 / -inf behind the last candidate. The result does not
 *   depend on the order of a candidate row's entries or on their repeats, bit for bit.
 *   The candidate CSR: cand_rowptr [n_query + 1], cand_colidx [cand_nnz], int32, on the device; row q belongs to QUERY q, not to a user: a
 *     user listed twice may carry two different rows. cand_nnz is the EXACT entry count, cand_rowptr[n_query].
 *   The exclusion CSR: the row rules of llmrec_score_topk_excluded_f32 (unsorted, repeats, padding; excl_rowptr == NULL with excl_nnz == 0:
 *     none). The train rows: ascending, duplicates allowed, as llmrec_csr_build leaves them.
 *   On the caller's one stream: (a) the error word is opened; (b) entry e of candidate row q (q by binary search in cand_rowptr) -> the
 *     64-bit key q << 32 | original id, a dropped entry -> n_query << 32, behind every row; the same launch checks cand_rowptr; (c) one radix
 *     sort of the keys (the vendor sort, between two buffers of the workspace, bits [0, 32 + bits of n_query)): rows in order, each
 *     ascending by id, repeats adjacent; (d) with an exclusion CSR, the keys kernel and the sort of the excluded call, identity numbering;
 *     (e) the score kernel: sorted key e is dropped if it equals key e - 1, is the dropped key, has its id in the train row of its user or
 *     has its key among the sorted exclusion keys (binary searches); otherwise its score is the k-ordered fp32 fma chain of
 *     llmrec_scores_f32 (for c, for s in 0..3, for q4 in 0..3: k = 16 c + 4 q4 + s, k < d, acc = fmaf(u[k], i[k], acc) from acc = +0), and
 *     the pair (q << 32 | ~m(score), id) goes out, m the order-preserving map of float bits to uint32; (f) one STABLE radix sort of the
 *     pairs over the same bits: its input ascends by id inside a query, so equal scores stay in id order (the chain never gives -0.0: equal
 *     floats are equal keys); (g) one wave per query: the lower bounds of q << 32 and (q + 1) << 32 in the sorted keys, the first
 *     min(K, count) ids and the scores decoded from the keys, -1 / -inf behind them.
 *     4 launches (5 with an exclusion CSR) + the sorts': a function of the host arguments alone; no allocation, no host read, no atomics,
 *     every cross-block hand-over a kernel boundary: capturable and deterministic. Tables are finite by contract: the rank of a NaN score
 *     is unspecified (nothing faults, nothing is written out of bounds).
 *   Caller errors the DEVICE detects - every list then comes back empty (-1 / -inf) and the call returns LLMREC_OK: a cand_rowptr or an
 *     excl_rowptr that does not start at 0, end at its nnz and never decrease.
 *   n_query == 0: no launch. cand_nnz == 0: one launch that fills the outputs; no workspace is needed.
 *   Bad sizes: LLMREC_EINVAL (the size function: -1), decided before any launch, as is a short workspace (LLMREC_EWORKSPACE).
 *   Workspace (16-byte aligned): llmrec_score_topk_candidates_workspace_bytes = 0 for n_query == 0 or cand_nnz == 0, else, with A(x) = x
 *     rounded up to 256,
 *       256 + 2 A(8 cand_nnz) + 2 A(4 cand_nnz) + A(cand_nnz + 32 MiB) + 2 A(8 excl_nnz) + [excl_nnz > 0: A(excl_nnz + 32 MiB)]
 *     (error word; two key buffers and two id buffers; the temporary storage of the two candidate sorts, the bound of the excluded call - a
 *     sort that asks for more is LLMREC_EWORKSPACE before the first launch; the exclusion stage's two key buffers and its reserve). The
 *     per-query bounds live in registers of the last launch: no buffer.
 * ------------------------------------------------------------------------------------------ */
int64_t llmrec_score_topk_candidates_workspace_bytes(int32_t n_query, int32_t K, int64_t cand_nnz, int64_t excl_nnz);
int llmrec_score_topk_candidates_f32(int32_t n_query, const int64_t* query_users,
                                     const float* Eu, int64_t ldu, const float* Ei, int64_t ldi, int64_t n_items, int32_t d,
                                     const int32_t* train_rowptr, const int32_t* train_colidx,
                                     int32_t K, int32_t* out_idx, float* out_score, void* workspace, int64_t workspace_bytes,
                                     const int32_t* cand_rowptr /* n_query + 1 */, const int32_t* cand_colidx, int64_t cand_nnz,
                                     const int32_t* excl_rowptr /* n_query + 1 or NULL */, const int32_t* excl_colidx, int64_t excl_nnz,
                                     const int32_t* new_id /* NULL = no filter */, llmrec_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Candidate lists under PER-GROUP QUOTAS (csrc/quota.hip): "at most m items of any one brand, seller, category or series in a user's list".
 * Additive: the ABI version stays, and no other prototype changes.
 *
 * llmrec_score_topk_candidates_capped_f32: the arguments of llmrec_score_topk_candidates_f32 with the same meaning, then
 *   item_group int32 [n_items] on the device: item_group[i] in [0, n_groups) is the group of item i; any other value (-1, >= n_groups) means
 *     NO GROUP, and such an item is never capped;
 *   the cap: group_cap int32 [n_groups] on the device, one cap >= 0 per group (0 removes the group), or group_cap == NULL and one cap >= 1 for
 *     every group (cap is not read beside a group_cap).
 *   Result: query q's survivors are those of the uncapped call (candidate row q as a set, minus ineligible items, minus the train row, minus
 *   exclusion row q), ranked by (score desc, ORIGINAL item id asc). The rank of a grouped item WITHIN ITS GROUP is the number of survivors
 *   of the same query and the same group that stand before it. An item is kept if it has no group or if that rank is below its group's
 *   cap; the list is the first K kept items, -1 / -inf behind the last one, the scores the bits of llmrec_scores_f32. This is the greedy
 *   walk down the ranking that takes an item while its group still has room. A cap at least as large as every group's survivor count
 *   gives the uncapped call's result, bit for bit. K <= LLMREC_TOPK_WIDE_MAX here: K sizes the group table of the last launch.
 *   On the caller's one stream: stages (a) to (f) of llmrec_score_topk_candidates_f32 - one internal function that both entries call: the
 *     same launches, the same buffers -, then (g') one wave per query: the query's range in the sorted keys as in (g), walked in chunks of
 *     64 sorted entries. Per chunk a lane's rank within its group = base[g] + the earlier lanes of the chunk with the same group; a ballot
 *     and a prefix popcount of the kept lanes give the output slot, a lane writes if its slot is below K, and the wave stops when K items
 *     are taken or the range ends. base[g] is a per-wave hash table in LDS keyed by group id, 2^s >= 2 K slots of 8 bytes (at most 32 KiB
 *     per block); only the first lane of a group within a chunk, and only if it is kept, adds the chunk's entries of the group to it (a
 *     group that is not kept any more has a count >= its cap in the table, or cap 0: nothing more is asked of it), so fewer than K slots
 *     are ever in use. Slots are claimed by integer LDS compare-and-swap; the counts read back do not depend on the table's layout.
 *     The launch count of the uncapped call: a function of the host arguments alone; no allocation, no host read, no global atomics, no
 *     float atomics: capturable and deterministic.
 *   Caller errors the DEVICE detects (a broken cand_rowptr / excl_rowptr): every list comes back empty and the call returns LLMREC_OK, as
 *     in the uncapped call. n_query == 0: no launch. cand_nnz == 0: one launch that fills the outputs; no workspace is needed.
 *   LLMREC_EINVAL before any launch: what the uncapped call refuses, K > LLMREC_TOPK_WIDE_MAX, item_group == NULL, n_groups < 1, and
 *     group_cap == NULL together with cap < 1. A short workspace: LLMREC_EWORKSPACE.
 *   Workspace: llmrec_score_topk_candidates_workspace_bytes(n_query, K, cand_nnz, excl_nnz), the uncapped call's - the table lives in LDS.
 * ------------------------------------------------------------------------------------------ */
int llmrec_score_topk_candidates_capped_f32(int32_t n_query, const int64_t* query_users,
                                            const float* Eu, int64_t ldu, const float* Ei, int64_t ldi, int64_t n_items, int32_t d,
                                            const int32_t* train_rowptr, const int32_t* train_colidx,
                                            int32_t K, int32_t* out_idx, float* out_score, void* workspace, int64_t workspace_bytes,
                                            const int32_t* cand_rowptr /* n_query + 1 */, const int32_t* cand_colidx, int64_t cand_nnz,
                                            const int32_t* excl_rowptr /* n_query + 1 or NULL */, const int32_t* excl_colidx, int64_t excl_nnz,
                                            const int32_t* new_id /* NULL = no filter */,
                                            const int32_t* item_group /* n_items */, int32_t n_groups, const int32_t* group_cap /* n_groups or NULL */,
                                            int32_t cap, llmrec_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Serving users who are NOT rows of the training graph (csrc/foldin.hip): the embedding the trained model gives a row of the
 * normalised adjacency that it has never seen, from the item-side tables alone. Additive: the ABI version stays.
 *
 * llmrec_fold_in_users_f32: n new users as a CSR over item ids (rowptr int32 [n + 1], colidx int32 [nnz], nnz = rowptr[n], on the
 *   device), row_scale float [n] (the caller's: D^-1/2 of the row), id_rows [n][d] through ldid or NULL (zeros), and ONE table
 *   T [n_items][C d] through ldt, C = L + 2 + n_attr + 1 slices of d columns:
 *       chain I_0 .. I_{L-1} | image | text | attribute 0 .. n_attr - 1 | profile.
 *   With S = the sum of T's rows at the entries of row r and g(c) = row_scale[r] * S[slice c]:
 *       out[r] = (id_rows[r] + g(0) + ... + g(L - 2) + softmax(g(L - 1))) * fl(1 / (L + 1))
 *                + c_m n(g(image)) + c_m n(g(text)) + c_u n(g(profile)) + sum_k c_a n(g(attribute k)),  n(x) = x / max(||x||_2, 1e-12),
 *   added in this order, the mean and the normalised terms with the operations of llmrec_fuse_fwd_f32.
 *   Entries < 0 or >= n_items add nothing (-1 padding; they do not change row_scale, which is the caller's); repeats count every time;
 *   an empty row gives zero sums and a uniform softmax row. A row whose pointers are no CSR row (outside 0 <= rowptr[r] <=
 *   rowptr[r + 1] <= nnz) counts as empty.
 *   The sum is fp32 in a fixed order that depends on the row's length alone: segments of 256 entries; inside a segment of len entries
 *   four runs of ceil(len / 4) consecutive entries, each added in the order given, meet as (r0 + r1) + (r2 + r3); the segments are
 *   added in order. No atomics: a row's bits do not depend on the other rows of the call, on its position in it, or on the run.
 *   One launch (every row of one segment is finished by the block that summed it); with nnz > 256 a second launch finishes the rows of
 *   more than one segment from the workspace. Grids come from n and nnz: no host read, capturable. Offsets into T are 64-bit.
 *   1 <= d <= 128, L >= 1, n_attr <= LLMREC_MAX_TERMS - 3, C d <= 2048 (else LLMREC_EUNSUPPORTED). float4 loads where d % 4 == 0,
 *   ldt % 4 == 0 and T is 16-byte aligned, scalar loads otherwise: the same sums, bit for bit.
 *   Workspace (16-byte aligned; too small: LLMREC_EWORKSPACE): llmrec_fold_in_users_workspace_bytes = 0 for nnz <= 256, else
 *   (n + floor(nnz / 256)) * C d * 4 - one [C d] slot per block; -1 for bad sizes.
 * ------------------------------------------------------------------------------------------ */
int64_t llmrec_fold_in_users_workspace_bytes(int32_t n, int64_t nnz, int32_t L, int32_t n_attr, int32_t d);
int llmrec_fold_in_users_f32(int32_t n, const int32_t* rowptr /* n + 1 */, const int32_t* colidx, int64_t nnz, const float* row_scale,
                             const float* id_rows, int64_t ldid, const float* T, int64_t ldt, int64_t n_items,
                             int32_t L, int32_t n_attr, int32_t d, float c_m, float c_u, float c_a,
                             float* out, int64_t ldo, void* workspace, int64_t workspace_bytes, llmrec_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * R11  on-device BPR sampler            replaces Data.sample (reference
 *                                        utility/load_data.py:157-195): B distinct users
 *                                        (keyed permutation of the users that have train items),
 *                                        one uniform positive from the user's CSR row, one
 *                                        uniform negative rejected while it is in that row.
 * Counter-based (Philox4x32-10) on (seed, step): reproducible and order-free.
 * ------------------------------------------------------------------------------------------ */
int llmrec_sample_bpr(uint64_t seed, uint64_t step, int64_t n_exist_users, const int64_t* exist_users,
                      int64_t n_items, const int32_t* train_rowptr, const int32_t* train_colidx,
                      int32_t B, int64_t* users, int64_t* pos, int64_t* neg, llmrec_stream_t stream);
/* The whole mini-batch of one step in one single-block launch a HIP graph can replay (the step counter is
 * device memory, advanced by the launch): slots [0, B) = this rank's slice [slice_begin, slice_begin + B) of
 * a global batch of B_global triples drawn exactly as llmrec_sample_bpr(seed, *step_dev, ..., B_global)
 * would; slots [B, B + n_aug) = the LLM-augmented triples of reference main.py:216-224 (n_aug distinct
 * users of the slice, their (aug_pos[u], aug_neg[u]) kept only if both are valid item ids; kept pairs first,
 * in draw order); n_valid_dev[0] = B + kept. users/pos/neg hold B + n_aug entries. */
int llmrec_sample_batch(uint64_t seed, uint64_t* step_dev, int64_t n_exist_users, const int64_t* exist_users,
                        int64_t n_items, const int32_t* train_rowptr, const int32_t* train_colidx,
                        int32_t B_global, int32_t slice_begin, int32_t B, int32_t n_aug,
                        const int64_t* aug_pos, const int64_t* aug_neg,
                        int64_t* users, int64_t* pos, int64_t* neg, int32_t* n_valid_dev, llmrec_stream_t stream);
/* The same batch, counter and n_valid by ceil(B / 256) + 1 blocks on as many CUs: 256 BPR slots per block, and one block that draws the
 * augmented triples on its own (it recomputes the users of its chosen slots instead of reading what the other blocks write). ticket:
 * one int32 of device memory, ZERO before the first call; every block increments it after its last use of *step_dev and the block that
 * draws the last ticket advances *step_dev and puts the ticket back to 0 (no block waits for another; graph replays need no host
 * action). One ticket word per sampler: calls that share it must be ordered on a stream. */
int llmrec_sample_batch_wide(uint64_t seed, uint64_t* step_dev, int64_t n_exist_users, const int64_t* exist_users,
                             int64_t n_items, const int32_t* train_rowptr, const int32_t* train_colidx,
                             int32_t B_global, int32_t slice_begin, int32_t B, int32_t n_aug,
                             const int64_t* aug_pos, const int64_t* aug_neg,
                             int64_t* users, int64_t* pos, int64_t* neg, int32_t* n_valid_dev, int32_t* ticket, llmrec_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * R12  dropout on the projections        replaces nn.Dropout on the eight projected feature
 *                                        tensors (reference Models.py:145-150) in the fused step,
 *                                        and its backward (the same mask on the gradient).
 * In-place inverted dropout of the row-major [rows, cols] view X (any ldx >= cols, any 4-byte-aligned
 * base; columns [cols, ldx) are never read or written). The mask is NOT torch's stream: it is this pure
 * function of (seed, step, tensor_tag, row, column), which a test can restate from these lines alone.
 *   generator  Philox4x32-10 (Salmon et al., SC'11; multipliers 0xD2511F53 / 0xCD9E8D57, key increments
 *              0x9E3779B9 / 0xBB67AE85), as the sampler above.
 *   key        k = seed ^ 0xD1B54A32D192ED03; key word 0 = low 32 bits of k, key word 1 = high 32 bits
 *              (a stream of its own: the sampler's keys are seed and seed ^ 0x9E3779B97F4A7C15).
 *   counter    (c >> 2, r, (uint32) s, (uint32) (s >> 32) * 256 + tensor_tag)   [the last word mod 2^32]
 *              for the element in row r, column c, with s = *step_dev as the launch reads it. The element
 *              uses output word c & 3 of that call: one call serves four consecutive columns.
 *   keep rule  the element is kept iff word >= T, T = (uint32) llrint((double) p * 4294967296.0) computed
 *              on the host and clamped to [1, 2^32 - 1].
 *   values     kept: x * scale with scale = 1.0f / (1.0f - p), both in fp32 (one rounding each);
 *              dropped: +0.0f exactly, whatever x was (a NaN or an infinity included).
 * LLMREC_EINVAL, before any HIP call, for: p outside (0, 1) or NaN; cols < 1; tensor_tag outside [0, 256);
 * rows < 0 or rows >= 2^32; with rows > 0, a null X or step_dev, a base that is not 4-byte aligned or
 * ldx < cols. rows == 0 succeeds without a launch.
 * The step counter is device memory, so a replayed graph follows it. ticket == NULL: the launch only READS
 * *step_dev. Otherwise ticket is one int32 of device memory, ZERO before the first call: every block
 * increments it after its last read of *step_dev, and the block that draws the last ticket adds 1 to
 * *step_dev and puts the ticket back to 0 (the count-off of llmrec_sample_batch_wide: no float atomics, no
 * block waits for another, no host action between replays). The caller orders the ticketed launch behind
 * every other reader of the counter in that step. tensor_tag names the tensor, so that tensors of one step
 * draw independent masks; the tags the fused step uses are in llmrec_amd/ops.py.
 * ------------------------------------------------------------------------------------------ */
int llmrec_dropout_rows_f32(int64_t rows, int32_t cols, float* X, int64_t ldx, float p,
                            uint64_t seed, uint64_t* step_dev, int32_t tensor_tag,
                            int32_t* ticket /* NULL: do not advance */, llmrec_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * R13  feature masking and attribute restoration   replaces MM_Model's in-place masking (reference
 *                                        Models.py:130-142) and the restoration term of the loss
 *                                        (main.py:258-273) in the fused step (opt-in).
 * The node lists are NOT torch.randperm's: they are the pure function below of (seed, round, side).
 *
 * llmrec_mask_nodes: nodes[j] = keyed_perm(j, N) for j < m - m distinct ids below N.
 *   keyed_perm  the sampler's keyed bijection of [0, N) (R11): a 4-round balanced Feistel network on 2 h bits, h the smallest
 *               h >= 1 with 4^h >= N; round r's function = the low h bits of the 64-bit word o[1] << 32 | o[0] of Philox4x32-10 at
 *               the counter (R low word, R high word ^ (0xA5A50000 + r), w low word, w high word); cycle-walk while the image is >= N.
 *   key         k = seed ^ 0x6A09E667F3BCC908 (key words: k low, k high) - beside the sampler's seed and
 *               seed ^ 0x9E3779B97F4A7C15 and the dropout's seed ^ 0xD1B54A32D192ED03.
 *   w           (2 s + side) mod 2^64, s = *step_dev as the launch reads it (the mask round); side = LLMREC_MASK_SIDE_USERS (0) or
 *               LLMREC_MASK_SIDE_ITEMS (1).
 *   ticket      NULL: the launch only READS *step_dev. Else one int32 of device memory, ZERO before the first call: the count-off of
 *               llmrec_sample_batch_wide - the block that draws the last ticket adds 1 to *step_dev and puts the ticket back to 0. The
 *               caller orders the ticketed launch behind the round's other reader. m == 0 with a ticket still advances the counter.
 * LLMREC_EINVAL before any HIP call: N < 1 or N >= 2^40; m < 0 or m > N; another side; a null step_dev; a null nodes with m > 0.
 *
 * llmrec_col_sums_f64 / llmrec_mask_rows_f32 act on n_tensors (1 .. LLMREC_MASK_MAX_TENSORS) row-major [N, cols] fp32 views with ONE
 * ldx >= cols (columns [cols, ldx) are never read or written; 64-bit element offsets) and one fp64 array sums[cols] each. X_host /
 * sums_host are HOST arrays of device pointers, read during the call.
 *   col_sums    sums[c] = the sum of column c in this tree, whatever the grid: row lane j (j < LLMREC_MASK_ROW_LANES = 8) adds rows
 *               j, j + 8, j + 16, ... in ascending order, in fp64, from +0.0; then ((((((l0 + l1) + l2) + l3) + l4) + l5) + l6) + l7.
 *   mask_rows   one round, per tensor and column c, every operation in fp64 rounded once (no fused multiply-add):
 *                 mean = (float) (sums[c] / (double) N)               [round to nearest even]
 *                 old  = the sum of X[nodes[i]][c] over i < m in col_sums' tree over the LIST POSITIONS i (lane j: i = j, j + 8, ...)
 *                 X[nodes[i]][c] = mean for every i < m
 *                 sums[c] = sums[c] + ((double) m * (double) mean - old)
 *               The nodes are read from device memory and must be distinct ids in [0, N) (llmrec_mask_nodes' are); nothing checks
 *               them. m == 0 succeeds without a launch.
 * LLMREC_EINVAL before any HIP call: n_tensors outside [1, 8]; N < 1; cols < 1; ldx < cols; m < 0 or m > N; a null array or entry;
 * a tensor base that is not 4-byte aligned or sums that are not 8-byte aligned; a null nodes with m > 0.
 *
 * llmrec_restore_loss_f32: n_streams (1 .. 8) streams share the node list, the decoder y = W x + b (W [F, d] row-major with ldw,
 * b [F]; LeakyReLU(True) has slope 1: the identity) and the loss. Stream s reads the rows x_r = X_host[s][nodes[r]][0 .. d) and the
 * targets t_r = T_host[s][nodes[r]][0 .. F), r < m, and returns
 *   row_loss[s m + r]   LLMREC_RESTORE_SCE: (1 - cos_r)^alpha;   LLMREC_RESTORE_MSE: (yy / ny^2 + tt / nt^2 - 2 cos_r) / F
 *                       with yy = y.y, yt = y.t, tt = t.t, ny = max(sqrt(yy), 1e-12f), nt = max(sqrt(tt), 1e-12f) (F.normalize's eps),
 *                       cos_r = yt / (ny nt);
 *   loss_out[s]         the 1024-slot tree of llmrec_bpr_multi_losses_assemble_f32 over row_loss[s m ..], divided by (float) m:
 *                       mean_r (1 - cos)^alpha, resp. F.mse_loss(normalize(y), normalize(t));
 *   dX_host != NULL     dX_host[s][nodes[r]][k] += scale * (cb p[k] + ca q[k]),  p = W^T y_r, q = W^T t_r  (= scale * dL_s / dx_r):
 *                         SCE  g = alpha (1 - cos)^(alpha - 1) / m;  ca = -g / (ny nt);  cb = g cos / ny^2, or 0 where sqrt(yy) < 1e-12f
 *                         MSE  g = 2 / (m F);                        ca = -g / (ny nt);  cb = g cos / ny^2, or g / ny^2 there
 *                       The node list must be duplicate-free (each destination row is read and written by one wavefront).
 *                       NULL: value only, nothing but row_loss / loss_out (and the flags) is written.
 *   row_flags           with row_stamp (both or neither): row_flags[nodes[r]] = LLMREC_ROW_STAMP(*row_stamp) - the rows join the
 *                       step's stamped rows, so llmrec_fuse_bwd_src_multi_f32 reads their sources.
 * Arithmetic: exact fp32, v_mfma_f32_16x16x4_f32 fma chains, no [rows, F] intermediate in memory. y[f] is the chain over
 * k = 16 j + 4 q + c in the order j, c, q (dense.hip's) plus b[f]; yy / yt / tt are, per lane, an fma chain over f = 16 n + 4 l + i
 * (n, then i, ascending) for l = 0 .. 3, combined (l0 + l1) + (l2 + l3); p[k] and q[k] are fma chains over f in the order n, i, l.
 * alpha 1, 2, 3 are products, any other value powf.
 * LLMREC_EINVAL before any HIP call: n_streams outside [1, 8]; m < 1 (the mean over an empty list is the reference's NaN: such a
 * step is not the library's) or m >= 2^31; F < 1; d < 1; another loss_type; alpha outside [1, 64] or NaN; a null nodes, W, b, row_loss,
 * loss_out, X_host, T_host or entry; one of row_flags / row_stamp without the other; ldx < d, ldt < F, ldw < d, lddx < d; a base that
 * is not 4-byte aligned. LLMREC_EUNSUPPORTED (nothing launched): d != 64.
 *
 * llmrec_restore_finish_f32: ONE launch behind the step's readers of both. (1) with n_values > 0: tot = ((v0 + v1) + ...) in fp32,
 * add = rate * tot; scal4[1] += add and running_sums3[0] += (double) add (either may be NULL). (2) with n_views > 0 and m > 0:
 * columns [0, cols) of the rows nodes[0 .. m) of every view (one ld) become +0.0f. LLMREC_EINVAL: n_values outside [0, 16] or
 * without values; n_views outside [0, 8]; m < 0; with views to clear, a null pointer, cols < 1 or ld < cols.
 * ------------------------------------------------------------------------------------------ */
#define LLMREC_MASK_ROW_LANES 8
#define LLMREC_MASK_MAX_TENSORS 8
#define LLMREC_MASK_SIDE_USERS 0
#define LLMREC_MASK_SIDE_ITEMS 1
#define LLMREC_RESTORE_SCE 0
#define LLMREC_RESTORE_MSE 1
int llmrec_mask_nodes(int64_t N, int64_t m, uint64_t seed, uint64_t* step_dev, int32_t side, int64_t* nodes,
                      int32_t* ticket /* NULL: do not advance */, llmrec_stream_t stream);
int llmrec_col_sums_f64(int32_t n_tensors, const float* const* X_host, int64_t ldx, double* const* sums_host, int64_t N, int32_t cols,
                        llmrec_stream_t stream);
int llmrec_mask_rows_f32(int32_t n_tensors, float* const* X_host, int64_t ldx, double* const* sums_host, int64_t N, int32_t cols,
                         const int64_t* nodes, int64_t m, llmrec_stream_t stream);
int llmrec_restore_loss_f32(int32_t n_streams, const float* const* X_host, int64_t ldx, const float* const* T_host, int64_t ldt,
                            float* const* dX_host /* NULL: value only */, int64_t lddx, const int64_t* nodes, int64_t m,
                            int32_t d, int32_t F, const float* W, int64_t ldw, const float* b, int32_t loss_type, float alpha, float scale,
                            float* row_loss, float* loss_out, uint8_t* row_flags, const int32_t* row_stamp, llmrec_stream_t stream);
int llmrec_restore_finish_f32(int32_t n_values, const float* values, float rate, float* scal4, double* running_sums3, int32_t n_views,
                              float* const* views_host, int64_t ld, int32_t cols, const int64_t* nodes, int64_t m, llmrec_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Checkpoint snapshot (csrc/snapshot.hip): n byte ranges ("segments") of device memory and ONE arena, moved by ONE launch whose
 * table of segments travels by value (no device-side table, no host synchronisation; capturable). Additive: the ABI version stays.
 *   llmrec_pack_arena_bytes  host arithmetic only, no device: offsets_host[i] = the offset of segment i in an arena that holds the
 *               segments in the given order, each at a multiple of LLMREC_PACK_ALIGN; returns the arena's size (a multiple of
 *               LLMREC_PACK_ALIGN; 0 for n == 0). Any n >= 0 (a caller with more than LLMREC_PACK_MAX_SEGMENTS segments lays out one
 *               arena and issues several launches over consecutive slices of it). -1: n < 0, a null array with n > 0, a negative
 *               size, a total beyond 2^63.
 *   llmrec_pack_segments   direction 0 (pack):   arena[offset[i] .. + bytes[i]) = ptr[i][0 .. bytes[i]) for every i, and EVERY other
 *                                                byte of arena[0 .. arena_bytes) = 0: equal states give byte-equal arenas;
 *                          direction 1 (unpack): ptr[i][0 .. bytes[i]) = arena[offset[i] .. + bytes[i]); nothing else is written.
 *               ptr_host / bytes_host / offset_host are HOST arrays read during the call; ptr[i] may have any alignment (16-byte
 *               aligned: 16 bytes per lane; 4-byte aligned: 4; else single bytes on the tensor side), all offsets are 64-bit.
 *               n == 0 with direction 0 zero-fills the arena.
 * LLMREC_EINVAL before any HIP call, nothing written: n outside [0, LLMREC_PACK_MAX_SEGMENTS]; a direction other than 0 or 1; a null
 * host array with n > 0; a null pointer with non-zero bytes; a negative size; an offset that is negative or not a multiple of
 * LLMREC_PACK_ALIGN; a segment that passes arena_bytes; arena_bytes < 0, a null arena with arena_bytes > 0 or an arena that is not
 * 16-byte aligned; direction 0 with two segments that overlap in the arena.
 * ------------------------------------------------------------------------------------------ */
#define LLMREC_PACK_MAX_SEGMENTS 64
#define LLMREC_PACK_ALIGN 256
int64_t llmrec_pack_arena_bytes(int32_t n, const int64_t* bytes_host, int64_t* offsets_host);
int llmrec_pack_segments(int32_t n, const void* const* ptr_host, const int64_t* bytes_host, const int64_t* offset_host,
                         void* arena, int64_t arena_bytes, int32_t direction, llmrec_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Measurement aid (bench.py `roofline`; nothing on the product path calls it). One single-lane launch that
 * stores the device's constant-rate real-time counter (s_memrealtime) into *slot when the stream reaches it.
 * A captured HIP graph cannot carry event-record nodes for external events; a pair of these around a launch
 * gives that launch's duration INSIDE the replayed graph. llmrec_timestamp_rate_hz: ticks per second of
 * that counter on the current device (hipDeviceAttributeWallClockRate), <= 0 on error.
 * ------------------------------------------------------------------------------------------ */
int llmrec_timestamp(uint64_t* slot, llmrec_stream_t stream);
int64_t llmrec_timestamp_rate_hz(void);

#ifdef __cplusplus
}
#endif
#endif /* LLMREC_HIP_H */
