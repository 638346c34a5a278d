// spmm.hip - R2: Y = epilogue(alpha * Z + diag(row_scale) * (P (.) val) * diag(col_scale) * X), fp32, CSR.
// Replaces torch.sparse.mm / torch.mm(sparse, dense) at reference Models.py:57-61 (call sites
// :153-157,162-163,166-167,176-180), the transposed SpMM autograd runs for the backward, and - as fused
// epilogues on the finished row - the row softmax of the last propagation layer (Models.py:176-177), its
// backward, and the "+ mean-term" additions of the hand-written backward (llmrec_amd/fused.py).
//
// HBM / fabric-bound gather kernel, organised for 64-lane wavefronts:
//   * a row of X / Y is d floats; LPR = d/4 lanes (16 for d = 64) each own one float4 of the row, so one
//     wavefront instruction moves 64/LPR complete rows as 16-byte-per-lane accesses (coalesced 256-B rows);
//   * CSR row buckets by length (llmrec_spmm_plan_*, thresholds chosen by the host), all in ONE launch of 512-thread
//     blocks, heaviest blocks first:
//       <= 32 nnz            one lane group per row (4 rows per wavefront at d = 64),
//       <= plan.t_wave       one wavefront per row (lane groups take contiguous parts, butterfly sum),
//       <= plan.t_block      one block (8 wavefronts) per row, waves summed through LDS in wave order,
//       longer               plan.segment-nnz segments, one block each, partial sums added in a fixed order by a second,
//                            tiny launch (only graphs with such hubs pay for it);
//     every summation tree is fixed by (nnz, thresholds, d): results are run-to-run deterministic, no float atomics.
//     (A ticket scheme - the last piece's wave sums the partials behind agent-scope fences, no second launch - was
//     measured and dropped: buffer_wbl2 writes back EVERY dirty line of the XCD's L2, 2.4x slower at 36 M edges and
//     3x slower in situ at Netflix scale, where concurrent kernels keep the L2 dirty.)
//   * wide operands ([rows, 7 x 64] side-feature blocks) can be cut into 64-column SLICES: (row, slice) tasks, so a
//     launch-bound graph gets 7x the parallelism and the latency of a d = 64 product instead of one wave per row;
//   * a lane group loads LPR column indices with one coalesced access and broadcasts them with ds_bpermute
//     (__shfl), then issues UNROLL independent row gathers before accumulating (UNROLL x 16 B in flight per lane);
//   * the adjacency values are not read at all in the reference's case (A = diag(s) R, R binary): a per-row
//     scale is applied once at the end (4 B/nnz of traffic instead of 8-20 B/nnz).
// What bounds it at scale (tools/gatherbench.py, profiles/r02_gatherbench_*.txt): the L2-miss path of the fabric,
// ~7.4 TB/s of 128-B lines from the Infinity Cache or HBM alike, plus ~25 TB/s for the L2 hits; a constant-degree
// graph without any imbalance reaches 35 G gathers/s on the synthetic graphs' popularity - this kernel's ceiling.
#include "common.h"
#include "guests.h"
#include "spmm_body.h"
#include <type_traits>

namespace llmrec {

// ONE launch of one problem (blk_begin = 0, blk_end = the grid).
template <int LPR, int NCHUNK, int VEC, bool WEIGHTED, bool MASKED>
__global__ __launch_bounds__(TPB) void spmm_kernel(SpmmArgs a) {
    constexpr int ROWW = NCHUNK * LPR * VEC;
    __shared__ __attribute__((aligned(16))) float red_lds[(TPB / 64 - 1) * ROWW];
    spmm_body<LPR, NCHUNK, VEC, WEIGHTED, MASKED>(a, (int32_t)blockIdx.x, red_lds);
}

// The slice-masked product (SpmmArgs.smask), weighted: an instance of its own, so the kernels above keep their registers.
template <int LPR, int NCHUNK, int VEC>
__global__ __launch_bounds__(TPB, 5) void spmm_smask_kernel(SpmmArgs a) {
    constexpr int ROWW = NCHUNK * LPR * VEC;
    __shared__ __attribute__((aligned(16))) float red_lds[(TPB / 64 - 1) * ROWW];
    spmm_body<LPR, NCHUNK, VEC, true, false, true>(a, (int32_t)blockIdx.x, red_lds);
}

// Up to LLMREC_SPMM_MAX_PROBLEMS independent problems of ONE kernel instance in one launch (llmrec_spmm_multi_f32): problem q owns the
// blocks [begin[q], begin[q + 1]). The arguments stay in the kernarg segment: a problem is picked by uniform compares and a switch over
// compile-time indices (a runtime index into p[] would copy the array to scratch).
struct SpmmMulti {
    SpmmArgs p[LLMREC_SPMM_MAX_PROBLEMS];
    int32_t begin[LLMREC_SPMM_MAX_PROBLEMS];     // first block of each problem; INT32_MAX past the last one
};
static_assert(sizeof(SpmmMulti) < 2048, "spmm: the grouped launch's kernarg block must stay well under 4 KB");

__device__ __forceinline__ int spmm_multi_problem(const SpmmMulti& m, int32_t b) {
    static_assert(LLMREC_SPMM_MAX_PROBLEMS == 4, "spmm_multi_problem picks one of four problems");
    return (int)(b >= m.begin[1]) + (int)(b >= m.begin[2]) + (int)(b >= m.begin[3]);
}

template <int LPR, int NCHUNK, int VEC, bool WEIGHTED, bool MASKED>
__global__ __launch_bounds__(TPB) void spmm_multi_kernel(SpmmMulti m) {
    constexpr int ROWW = NCHUNK * LPR * VEC;
    __shared__ __attribute__((aligned(16))) float red_lds[(TPB / 64 - 1) * ROWW];
    const int32_t b = blockIdx.x;
    switch (spmm_multi_problem(m, b)) {                                   // (block-uniform)
    case 0: spmm_body<LPR, NCHUNK, VEC, WEIGHTED, MASKED>(m.p[0], b, red_lds); break;
    case 1: spmm_body<LPR, NCHUNK, VEC, WEIGHTED, MASKED>(m.p[1], b, red_lds); break;
    case 2: spmm_body<LPR, NCHUNK, VEC, WEIGHTED, MASKED>(m.p[2], b, red_lds); break;
    default: spmm_body<LPR, NCHUNK, VEC, WEIGHTED, MASKED>(m.p[3], b, red_lds); break;
    }
}

// the grouped launch of the slice-masked instance: members without a mask carry smask_col0 = their width and run the plain loops
template <int LPR, int NCHUNK, int VEC>
__global__ __launch_bounds__(TPB, 5) void spmm_smask_multi_kernel(SpmmMulti m) {
    constexpr int ROWW = NCHUNK * LPR * VEC;
    __shared__ __attribute__((aligned(16))) float red_lds[(TPB / 64 - 1) * ROWW];
    const int32_t b = blockIdx.x;
    switch (spmm_multi_problem(m, b)) {                                   // (block-uniform)
    case 0: spmm_body<LPR, NCHUNK, VEC, true, false, true>(m.p[0], b, red_lds); break;
    case 1: spmm_body<LPR, NCHUNK, VEC, true, false, true>(m.p[1], b, red_lds); break;
    case 2: spmm_body<LPR, NCHUNK, VEC, true, false, true>(m.p[2], b, red_lds); break;
    default: spmm_body<LPR, NCHUNK, VEC, true, false, true>(m.p[3], b, red_lds); break;
    }
}

// The grouped launch with a GUEST (llmrec_spmm_multi_guest_f32): blocks [0, guest_blocks) run the guest's body (guests.h: the sampler,
// the scatter plan + reach marks, or the loss values, in their 512-thread forms), the problems' ranges follow (begin[0] = guest_blocks).
// The guest depends on nothing this launch computes and nothing here waits for it: its short blocks, which a launch of their own would
// run on a few CUs of an otherwise idle chip, start first and the latency-bound products fill the rest. Only the step's instance is
// compiled (16 lanes per row, float4, one chunk); one kernel per guest kind, so each keeps the registers of its own body only.
template <class G>
struct SpmmMultiGuest {
    SpmmMulti m;
    int32_t guest_blocks;
    G g;
};

// Each instance is held to its host spmm_kernel's waves per SIMD (7 unweighted, 5 weighted): inlined, the sampler's Philox rounds would
// otherwise cost the unweighted host two registers and with them the seventh wave (73 VGPRs against 71).
template <bool WEIGHTED, class G>
__global__ __launch_bounds__(TPB, WEIGHTED ? 5 : 7) void spmm_multi_guest_kernel(SpmmMultiGuest<G> m) {
    constexpr int LPR = 16, NCHUNK = 1, VEC = 4, ROWW = NCHUNK * LPR * VEC;
    __shared__ __attribute__((aligned(16))) float red_lds[(TPB / 64 - 1) * ROWW];
    extern __shared__ __attribute__((aligned(16))) char guest_lds[];
    const int32_t b = blockIdx.x;
    if (b < m.guest_blocks) {                                             // (block-uniform)
        guest_block<TPB>(m.g, b, guest_lds);
        return;
    }
    switch (spmm_multi_problem(m.m, b)) {                                 // (block-uniform)
    case 0: spmm_body<LPR, NCHUNK, VEC, WEIGHTED, false>(m.m.p[0], b, red_lds); break;
    case 1: spmm_body<LPR, NCHUNK, VEC, WEIGHTED, false>(m.m.p[1], b, red_lds); break;
    case 2: spmm_body<LPR, NCHUNK, VEC, WEIGHTED, false>(m.m.p[2], b, red_lds); break;
    default: spmm_body<LPR, NCHUNK, VEC, WEIGHTED, false>(m.m.p[3], b, red_lds); break;
    }
}

// the guest launch of the slice-masked instance (the backward's first group hosts the loss values: compiled for that guest only)
template <class G>
__global__ __launch_bounds__(TPB, 5) void spmm_smask_multi_guest_kernel(SpmmMultiGuest<G> m) {
    constexpr int LPR = 16, NCHUNK = 1, VEC = 4, ROWW = NCHUNK * LPR * VEC;
    __shared__ __attribute__((aligned(16))) float red_lds[(TPB / 64 - 1) * ROWW];
    extern __shared__ __attribute__((aligned(16))) char guest_lds[];
    const int32_t b = blockIdx.x;
    if (b < m.guest_blocks) {                                             // (block-uniform)
        guest_block<TPB>(m.g, b, guest_lds);
        return;
    }
    switch (spmm_multi_problem(m.m, b)) {                                 // (block-uniform)
    case 0: spmm_body<LPR, NCHUNK, VEC, true, false, true>(m.m.p[0], b, red_lds); break;
    case 1: spmm_body<LPR, NCHUNK, VEC, true, false, true>(m.m.p[1], b, red_lds); break;
    case 2: spmm_body<LPR, NCHUNK, VEC, true, false, true>(m.m.p[2], b, red_lds); break;
    default: spmm_body<LPR, NCHUNK, VEC, true, false, true>(m.m.p[3], b, red_lds); break;
    }
}

template <int LPR, int NCHUNK, int VEC>
__global__ __launch_bounds__(256) void spmm_finalize_kernel(SpmmArgs a) {
    __shared__ __attribute__((aligned(16))) float fin_lds[(256 / LPR) * NCHUNK * LPR * VEC];
    spmm_finalize_body<LPR, NCHUNK, VEC>(a, (int32_t)blockIdx.x, fin_lds);
}

// the grouped launch's finalize: problem q owns the blocks [begin[q], begin[q + 1]) (its split rows x slices)
template <int LPR, int NCHUNK, int VEC>
__global__ __launch_bounds__(256) void spmm_finalize_multi_kernel(SpmmMulti m) {
    __shared__ __attribute__((aligned(16))) float fin_lds[(256 / LPR) * NCHUNK * LPR * VEC];
    const int32_t b = blockIdx.x;
    switch (spmm_multi_problem(m, b)) {                                   // (block-uniform)
    case 0: spmm_finalize_body<LPR, NCHUNK, VEC>(m.p[0], b - m.begin[0], fin_lds); break;
    case 1: spmm_finalize_body<LPR, NCHUNK, VEC>(m.p[1], b - m.begin[1], fin_lds); break;
    case 2: spmm_finalize_body<LPR, NCHUNK, VEC>(m.p[2], b - m.begin[2], fin_lds); break;
    default: spmm_finalize_body<LPR, NCHUNK, VEC>(m.p[3], b - m.begin[3], fin_lds); break;
    }
}

// "These rows of A X" with the list and its length on the device (llmrec_spmm_rows_compact_f32): block (j, p) sums piece p of listed row j
// (block_range: 8 waves, LDS reduction in wave order) into partial[j][p]; rows up to COMPACT_MIN_PIECE nnz are one piece.
constexpr int COMPACT_MIN_PIECE = 2048;
__device__ __forceinline__ void compact_pieces(int32_t deg, int32_t& per, int32_t& n_pieces) {
    per = (deg + LLMREC_SPMM_COMPACT_PARTS - 1) / LLMREC_SPMM_COMPACT_PARTS;
    per = (per + 511) / 512 * 512;                                    // (whole 64-index chunks per wave)
    if (per < COMPACT_MIN_PIECE) per = COMPACT_MIN_PIECE;
    n_pieces = deg > 0 ? (deg + per - 1) / per : 0;
}
template <int LPR, int NCHUNK, int VEC>
__global__ __launch_bounds__(TPB) void spmm_rows_compact_kernel(SpmmArgs a, const int32_t* __restrict__ row_list, const int32_t* __restrict__ n_list,
                                                                float* __restrict__ partial) {
    constexpr int ROWW = NCHUNK * LPR * VEC;
    __shared__ __attribute__((aligned(16))) float red_lds[(TPB / 64 - 1) * ROWW];
    const int j = blockIdx.x, p = blockIdx.y;
    if (j >= n_list[0]) return;                                         // block-uniform
    const int32_t row = row_list[j];
    const int32_t s = a.rowptr[row], e = a.rowptr[row + 1];
    int32_t per, n_pieces;
    compact_pieces(e - s, per, n_pieces);
    if (p >= n_pieces) return;
    Vec<VEC> acc[NCHUNK];
    if (block_range<LPR, NCHUNK, VEC, false, false>(a, 0, s + p * per, min(s + (p + 1) * per, e), red_lds, acc, nullptr, 0)) {
        float* pr = partial + ((int64_t)j * LLMREC_SPMM_COMPACT_PARTS + p) * a.d;
#pragma unroll
        for (int k = 0; k < NCHUNK; ++k) {
            const int col = (k * LPR + (int)threadIdx.x) * VEC;
            if (col < a.d) acc[k].store(pr + col);
        }
    }
}
// one lane group per slot j < capacity: the pieces of row j in piece order, the row scale; zeros past the list's end
template <int LPR, int NCHUNK, int VEC>
__global__ __launch_bounds__(256) void spmm_rows_compact_finish_kernel(SpmmArgs a, const int32_t* __restrict__ row_list, const int32_t* __restrict__ n_list,
                                                                       int capacity, const float* __restrict__ partial, float* __restrict__ out, int64_t ldo) {
    const int gl = threadIdx.x & (LPR - 1);
    const int j = blockIdx.x * (256 / LPR) + threadIdx.x / LPR;
    if (j >= capacity) return;
    Vec<VEC> acc[NCHUNK];
#pragma unroll
    for (int k = 0; k < NCHUNK; ++k) acc[k].zero();
    float rs = 0.f;
    if (j < n_list[0]) {
        const int32_t row = row_list[j];
        int32_t per, n_pieces;
        compact_pieces(a.rowptr[row + 1] - a.rowptr[row], per, n_pieces);
        for (int p = 0; p < n_pieces; ++p) {
            const float* pr = partial + ((int64_t)j * LLMREC_SPMM_COMPACT_PARTS + p) * a.d;
#pragma unroll
            for (int k = 0; k < NCHUNK; ++k) {
                const int col = (k * LPR + gl) * VEC;
                if (col < a.d) { Vec<VEC> v; v.load(pr + col); acc[k].add(v); }
            }
        }
        rs = a.row_scale ? a.row_scale[row] : 1.0f;
    }
#pragma unroll
    for (int k = 0; k < NCHUNK; ++k) {
        const int col = (k * LPR + gl) * VEC;
        acc[k].scale(rs);
        if (col < a.d) acc[k].store(out + (int64_t)j * ldo + col);
    }
}

template <int LPR, int NCHUNK, int VEC>
static int launch_rows_compact(SpmmArgs& a, const int32_t* row_list, const int32_t* n_list, int capacity, float* out, int64_t ldo, float* partial,
                               hipStream_t stream) {
    spmm_rows_compact_kernel<LPR, NCHUNK, VEC><<<dim3((unsigned)capacity, LLMREC_SPMM_COMPACT_PARTS), TPB, 0, stream>>>(a, row_list, n_list, partial);
    LLMREC_LAUNCH_CHECK();
    spmm_rows_compact_finish_kernel<LPR, NCHUNK, VEC><<<(unsigned)ceil_div(capacity, 256 / LPR), 256, 0, stream>>>(a, row_list, n_list, capacity, partial, out, ldo);
    LLMREC_LAUNCH_CHECK();
    return LLMREC_OK;
}

// The compiled kernel family (LPR, NCHUNK, VEC) and variant (WEIGHTED, MASKED) of a product: two products can share a grouped launch
// only when both agree. The grouped kernels are compiled for the vector-load families (0..6) and the unmasked variants: the latency-bound
// products of the step; masked products run in the HBM-bound or row-restricted paths.
// SPMM_V_SMASK_W: the slice-masked weighted product (x_mask_stamp) - family 2 only, single, grouped and as the loss values' host.
enum { SPMM_V_MASKED_W, SPMM_V_MASKED, SPMM_V_WEIGHTED, SPMM_V_PLAIN, SPMM_V_SMASK_W };
static const int kSpmmFamilyLpr[] = {4, 8, 16, 32, 64, 64, 64, 16, 64, 64};

struct SpmmPrepared {
    SpmmArgs a;
    int family, variant;
    bool empty;                                  // n_rows == 0 or d == 0: nothing to launch
    int64_t bytes_x, bytes_y, bytes_z, bytes_s, bytes_partials;     // extents, for the grouped launch's aliasing check
};

static int64_t extent_bytes(int64_t rows, int64_t ld, int64_t width) { return rows > 0 && width > 0 ? ((rows - 1) * ld + width) * 4 : 0; }

// The argument checks and the SpmmArgs of one product (llmrec_spmm_f32 and each problem of llmrec_spmm_multi_f32).
static int spmm_prepare(const llmrec_spmm_problem_t& pr, SpmmPrepared& out) {
    const int64_t n_rows = pr.n_rows, n_cols = pr.n_cols, ldx = pr.ldx, ldy = pr.ldy;
    const int32_t d = pr.d, slice_width = pr.slice_width;
    const float* X = pr.X;
    float* Y = pr.Y;
    float* partials = pr.partials;
    const llmrec_spmm_epilogue_t* epilogue_host = pr.epilogue;
    out = SpmmPrepared{};
    LLMREC_CHECK_ARG(n_rows >= 0 && n_cols >= 0 && d >= 0, "spmm: negative size");
    out.empty = n_rows == 0 || d == 0;
    if (out.empty) return LLMREC_OK;
    LLMREC_CHECK_ARG(pr.rowptr && Y && ldy >= d && ldx >= d, "spmm: null pointer or ld < d");
    LLMREC_CHECK_ARG(pr.plan, "spmm: a row plan is required (llmrec_spmm_plan_count / _fill)");
    const llmrec_spmm_plan_t& p = *pr.plan;
    LLMREC_CHECK_ARG(p.n_wave_rows >= 0 && p.n_block_rows >= 0 && p.n_split_rows >= 0 && p.n_segments >= 0 && p.segment >= LLMREC_SPMM_LONG_ROW,
                     "spmm: bad plan sizes");
    LLMREC_CHECK_ARG((p.n_wave_rows == 0 || p.wave_rows) && (p.n_block_rows == 0 || p.block_rows) &&
                     (p.n_split_rows == 0 || (p.split_rows && p.split_seg_begin && p.seg_split && partials)), "spmm: row plan incomplete");
    LLMREC_CHECK_ARG(slice_width == 0 || (slice_width > 0 && d % slice_width == 0), "spmm: slice_width must divide d");
    SpmmArgs& a = out.a;
    a.n_rows = n_rows; a.rowptr = pr.rowptr; a.colidx = pr.colidx; a.val = pr.val; a.row_scale = pr.row_scale;
    a.col_scale = pr.col_scale; a.X = X; a.ldx = ldx; a.Y = Y; a.ldy = ldy;
    a.d = slice_width > 0 ? slice_width : d;
    a.n_slices = slice_width > 0 ? d / slice_width : 1;
    a.wave_rows = p.wave_rows; a.block_rows = p.block_rows; a.split_rows = p.split_rows; a.split_seg_begin = p.split_seg_begin;
    a.seg_split = p.seg_split; a.partials = partials;
    LLMREC_CHECK_ARG(p.n_short_rows >= 0 && p.n_short_rows <= n_rows, "spmm: bad short-row count");
    LLMREC_CHECK_ARG(!p.slot_row || (!pr.val && !(epilogue_host && epilogue_host->rows_listed_only)), "spmm: a permuted CSR is pattern-only and complete");
    a.slot_row = p.slot_row; a.n_short_rows = p.slot_row ? p.n_short_rows : 0;
    a.n_wave_rows = p.n_wave_rows; a.n_block_rows = p.n_block_rows; a.n_split_rows = p.n_split_rows; a.n_segments = p.n_segments;
    a.segment = p.segment;
    a.epi_op = LLMREC_SPMM_EPI_NONE; a.alpha = 0.f;
    bool epi_aligned = true;
    if (epilogue_host) {
        const llmrec_spmm_epilogue_t& e = *epilogue_host;
        LLMREC_CHECK_ARG(e.op >= LLMREC_SPMM_EPI_NONE && e.op <= LLMREC_SPMM_EPI_SOFTMAX_BWD, "spmm: unknown epilogue op %d", e.op);
        LLMREC_CHECK_ARG(e.op == LLMREC_SPMM_EPI_NONE || a.n_slices == 1, "spmm: the softmax epilogues need the whole row (slice_width = 0)");
        LLMREC_CHECK_ARG(!e.Z || e.ldz >= d, "spmm: epilogue Z with ld < d");
        LLMREC_CHECK_ARG(e.op != LLMREC_SPMM_EPI_SOFTMAX_BWD || (e.S && e.lds >= d), "spmm: softmax backward needs S with ld >= d");
        a.epi_op = e.op; a.alpha = e.alpha; a.Z = e.Z; a.ldz = e.ldz; a.S = e.S; a.lds = e.lds; a.post_scale = e.post_scale;
        a.listed_only = e.rows_listed_only != 0;
        if (e.y_row_needed) {
            LLMREC_CHECK_ARG(e.x_mask_active >= 1 && e.x_mask_active <= 255, "spmm: y_row_needed needs x_mask_active in 1..255");
            a.y_needed = e.y_row_needed; a.x_active = e.x_mask_active;
        }
        if (e.x_mask_stamp) {
            // the slice-ranged mask with a device stamp: a kernel instance of its own, nothing of the host-stamped masks beside it
            LLMREC_CHECK_ARG(e.x_row_mask && e.mask_from_slice >= 0 && e.mask_from_slice <= a.n_slices, "spmm: x_mask_stamp needs x_row_mask and mask_from_slice in 0..%d", a.n_slices);
            LLMREC_CHECK_ARG(!e.y_row_flag && !e.z_row_flag && !e.y_row_gate && !e.y_row_needed && !e.rows_listed_only && e.op == LLMREC_SPMM_EPI_NONE,
                             "spmm: x_mask_stamp excludes the row flags, gates, row lists and the softmax epilogues");
            a.smask = e.x_row_mask; a.smask_stamp = e.x_mask_stamp; a.smask_col0 = e.mask_from_slice * a.d;
            a.smask_inplace = e.Z == Y && e.ldz == ldy && e.alpha == 1.0f && !e.post_scale;
        } else if (e.x_row_mask) {
            LLMREC_CHECK_ARG(e.x_mask_active >= 1 && e.x_mask_active <= 255, "spmm: x_mask_active must be a byte value 1..255");
            a.x_mask = e.x_row_mask; a.x_active = e.x_mask_active; a.y_flag = e.y_row_flag; a.z_flag = e.z_row_flag;
            LLMREC_CHECK_ARG(!e.y_row_gate || e.op != LLMREC_SPMM_EPI_SOFTMAX, "spmm: y_row_gate with the forward softmax (a zero row is not a zero output)");
            a.y_gate = e.y_row_gate;
        } else {
            LLMREC_CHECK_ARG(!e.y_row_flag, "spmm: y_row_flag needs x_row_mask");
        }
        epi_aligned = (!e.Z || (e.ldz % 4 == 0 && (uintptr_t)e.Z % 16 == 0)) && (!e.S || (e.lds % 4 == 0 && (uintptr_t)e.S % 16 == 0));
    }
    const int dd = a.d;
    const bool vec4 = (dd % 4 == 0) && (ldx % 4 == 0) && (ldy % 4 == 0) && epi_aligned &&
                      (((uintptr_t)X | (uintptr_t)Y | (uintptr_t)partials) % 16 == 0);
    int f = -1;
    if (vec4) f = dd <= 16 ? 0 : dd <= 32 ? 1 : dd <= 64 ? 2 : dd <= 128 ? 3 : dd <= 256 ? 4 : dd <= 512 ? 5 : dd <= 1024 ? 6 : -1;
    else f = dd <= 16 ? 7 : dd <= 64 ? 8 : dd <= 256 ? 9 : -1;
    if (f < 0) {
        set_error("spmm: d = %d outside the compiled kernel family (vec4 = %d)", dd, (int)vec4);
        return LLMREC_EUNSUPPORTED;
    }
    const bool weighted = a.val != nullptr || a.col_scale != nullptr;
    out.family = f;
    out.variant = a.x_mask ? (weighted ? SPMM_V_MASKED_W : SPMM_V_MASKED)
                : weighted ? SPMM_V_WEIGHTED : SPMM_V_PLAIN;
    if (a.smask) {
        const int64_t tasks = (p.slot_row ? (int64_t)p.n_short_rows : n_rows) * a.n_slices;
        const char* why = f != 2 ? "its slices are not float4 rows of 33..64 columns" : a.val ? "the operand has val" :
                          !a.col_scale ? "the operand has no col_scale" : tasks + (TPB / 16) * 8192 >= (1ll << 31) ? "too many (row, slice) tasks" : nullptr;
        if (why) {
            set_error("spmm: the slice-masked product is compiled for the pattern-only float4 products of 33..64 columns per slice weighted by col_scale: %s (family %d)", why, f);
            return LLMREC_EUNSUPPORTED;
        }
        out.variant = SPMM_V_SMASK_W;
    }
    out.bytes_x = X ? extent_bytes(n_cols, ldx, d) : 0;
    out.bytes_y = extent_bytes(n_rows, ldy, d);
    out.bytes_z = a.Z ? extent_bytes(n_rows, a.ldz, d) : 0;
    out.bytes_s = a.S ? extent_bytes(n_rows, a.lds, d) : 0;
    out.bytes_partials = partials ? (int64_t)p.n_segments * d * 4 : 0;
    return LLMREC_OK;
}

// The block ranges of one problem whose blocks start at `first` (0 for a launch of its own); returns its block count, -1 past 32-bit ids.
// tpb: the threads of a block of the launch (a product hosted by another kernel's launch runs in that kernel's blocks).
static int64_t spmm_layout(SpmmArgs& a, int lpr, int64_t first, int tpb = TPB) {
    const int64_t GPB = tpb / lpr;
    const int64_t S = a.n_slices;
    // unmasked products: the short rows' tasks as software pipelines (rows_body_pipe) - as many tasks per lane group as keep ~4 blocks per CU
    const int64_t short_tasks = a.listed_only ? 0 : (a.slot_row ? (int64_t)a.n_short_rows : a.n_rows) * S;
    int64_t pipe = 1;
    if (!a.x_mask) {
        pipe = short_tasks + GPB * 8192 < (1ll << 31) ? ceil_div(short_tasks, GPB * 1024) : 1;      // (32-bit task ids in the kernel)
        if (pipe > 8) pipe = 8;
        if (pipe < 1) pipe = 1;
    }
    a.pipe = (int32_t)pipe;
    const int64_t row_blocks = ceil_div(short_tasks, GPB * pipe);
    const int64_t wave_blocks = ceil_div(a.n_wave_rows * S, tpb / 64);
    const int64_t total = a.n_segments * S + a.n_block_rows * S + wave_blocks + row_blocks;
    if (first + total > 0x7fffffffll) return -1;
    a.blk_begin = (int32_t)first;
    a.blk_seg = a.blk_begin + (int32_t)(a.n_segments * S);
    a.blk_block = a.blk_seg + (int32_t)(a.n_block_rows * S);
    a.blk_wave = a.blk_block + (int32_t)wave_blocks;
    a.blk_end = (int32_t)(first + total);
    return total;
}

// One launch of n >= 1 laid-out problems of one family / variant (n == 1: the single-problem kernels), then the finalize launch of the
// problems with split rows.
// The guest of a grouped launch, checked and laid out (spmm_run): the kernel arguments of its kind, its blocks and its dynamic LDS.
struct GuestLaunch {
    int kind;
    SamplerArgs sampler;
    PlanReachArgs plan_reach;
    LossesArgs losses;
    int64_t blocks;
    size_t shmem;
};

template <class G>
static void launch_spmm_guest(int n, const SpmmPrepared* pp, int variant, int64_t total, const G& g, const GuestLaunch& gl, hipStream_t stream) {
    SpmmMultiGuest<G> m = {};
    for (int q = 0; q < LLMREC_SPMM_MAX_PROBLEMS; ++q) {
        if (q < n) { m.m.p[q] = pp[q].a; m.m.begin[q] = pp[q].a.blk_begin; }
        else m.m.begin[q] = 0x7fffffff;
    }
    m.guest_blocks = (int32_t)gl.blocks;
    m.g = g;
    if (variant == SPMM_V_SMASK_W) {
        if constexpr (std::is_same<G, LossesArgs>::value) spmm_smask_multi_guest_kernel<G><<<(unsigned)total, TPB, gl.shmem, stream>>>(m);   // (spmm_run: this guest only)
    } else if (variant == SPMM_V_WEIGHTED) spmm_multi_guest_kernel<true, G><<<(unsigned)total, TPB, gl.shmem, stream>>>(m);
    else spmm_multi_guest_kernel<false, G><<<(unsigned)total, TPB, gl.shmem, stream>>>(m);
}

template <int LPR, int NCHUNK, int VEC>
static int launch_spmm(int n, SpmmPrepared* pp, int variant, int64_t total, hipStream_t stream, const GuestLaunch* guest = nullptr) {
    if (total > 0) {
        if (guest) {                                         // (spmm_run: family 2, unmasked; total counts the guest's blocks)
            if (guest->kind == LLMREC_SPMM_GUEST_SAMPLER) launch_spmm_guest(n, pp, variant, total, guest->sampler, *guest, stream);
            else if (guest->kind == LLMREC_SPMM_GUEST_PLAN_REACH) launch_spmm_guest(n, pp, variant, total, guest->plan_reach, *guest, stream);
            else launch_spmm_guest(n, pp, variant, total, guest->losses, *guest, stream);
        } else if (variant == SPMM_V_SMASK_W) {              // (spmm_prepare: family 2 only)
            if constexpr (LPR == 16 && NCHUNK == 1 && VEC == 4) {
                if (n == 1) spmm_smask_kernel<LPR, NCHUNK, VEC><<<(unsigned)total, TPB, 0, stream>>>(pp[0].a);
                else {
                    SpmmMulti m = {};
                    for (int q = 0; q < LLMREC_SPMM_MAX_PROBLEMS; ++q) {
                        if (q < n) { m.p[q] = pp[q].a; m.begin[q] = pp[q].a.blk_begin; }
                        else m.begin[q] = 0x7fffffff;
                    }
                    spmm_smask_multi_kernel<LPR, NCHUNK, VEC><<<(unsigned)total, TPB, 0, stream>>>(m);
                }
            }
        } else if (n == 1) {
            const SpmmArgs& a = pp[0].a;
            switch (variant) {
            case SPMM_V_MASKED_W: spmm_kernel<LPR, NCHUNK, VEC, true, true><<<(unsigned)total, TPB, 0, stream>>>(a); break;
            case SPMM_V_MASKED: spmm_kernel<LPR, NCHUNK, VEC, false, true><<<(unsigned)total, TPB, 0, stream>>>(a); break;
            case SPMM_V_WEIGHTED: spmm_kernel<LPR, NCHUNK, VEC, true, false><<<(unsigned)total, TPB, 0, stream>>>(a); break;
            default: spmm_kernel<LPR, NCHUNK, VEC, false, false><<<(unsigned)total, TPB, 0, stream>>>(a); break;
            }
        } else if constexpr (VEC == 4) {                     // (spmm_run groups the vector-load families only)
            SpmmMulti m = {};
            for (int q = 0; q < LLMREC_SPMM_MAX_PROBLEMS; ++q) {
                if (q < n) { m.p[q] = pp[q].a; m.begin[q] = pp[q].a.blk_begin; }
                else m.begin[q] = 0x7fffffff;
            }
            if (variant == SPMM_V_WEIGHTED) spmm_multi_kernel<LPR, NCHUNK, VEC, true, false><<<(unsigned)total, TPB, 0, stream>>>(m);
            else spmm_multi_kernel<LPR, NCHUNK, VEC, false, false><<<(unsigned)total, TPB, 0, stream>>>(m);
        }
        LLMREC_LAUNCH_CHECK();
    }
    // split rows: their segment partials are summed in a fixed order by one more launch (one block per split row and slice)
    SpmmMulti fin = {};
    int nf = 0;
    int64_t fin_total = 0;
    for (int q = 0; q < n; ++q) {
        const SpmmArgs& a = pp[q].a;
        if (a.n_split_rows <= 0) continue;
        fin.p[nf] = a; fin.begin[nf] = (int32_t)fin_total;
        fin_total += (int64_t)a.n_split_rows * a.n_slices;
        ++nf;
    }
    if (nf == 1) {
        spmm_finalize_kernel<LPR, NCHUNK, VEC><<<(unsigned)fin_total, 256, 0, stream>>>(fin.p[0]);
        LLMREC_LAUNCH_CHECK();
    } else if constexpr (VEC == 4) {
        if (nf > 1) {
            for (int q = nf; q < LLMREC_SPMM_MAX_PROBLEMS; ++q) fin.begin[q] = 0x7fffffff;
            spmm_finalize_multi_kernel<LPR, NCHUNK, VEC><<<(unsigned)fin_total, 256, 0, stream>>>(fin);
            LLMREC_LAUNCH_CHECK();
        }
    }
    return LLMREC_OK;
}

static bool bytes_overlap(const void* p, int64_t np, const void* q, int64_t nq) {
    if (!p || !q || np <= 0 || nq <= 0) return false;
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + (uintptr_t)nq && b < a + (uintptr_t)np;
}

// One product for the launch of ANOTHER kernel that hosts it in blocks of `tpb` threads (spmm_body.h: spmm_hosted_body; dense.hip's
// grouped projection and multi-target weight gradient): the checks of spmm_prepare, then the two narrow shapes the hosted body is
// compiled for, laid out from block 0 - the plain whole-row product without an epilogue, and the product weighted by col_scale alone
// whose only epilogue is the init term alpha Z (finish_row applies it at run time). out.weighted says which; each host takes one.
// LLMREC_EUNSUPPORTED for anything else - the caller has launched nothing yet.
int spmm_prepare_hosted(const llmrec_spmm_problem_t& pr, int tpb, SpmmHosted& out) {
    SpmmPrepared pp;
    const int rc = spmm_prepare(pr, pp);
    if (rc != LLMREC_OK) return rc;
    const SpmmArgs& a = pp.a;
    const bool weighted = pp.variant == SPMM_V_WEIGHTED;
    const char* why = pp.empty ? "the product is empty" : pp.family != 2 ? "not a float4 product of 33..64 columns" :
                      (pp.variant != SPMM_V_PLAIN && !weighted) ? "the operand has a mask" : a.val ? "the operand has val" :
                      a.n_slices != 1 ? "column slices" : a.n_split_rows > 0 ? "the plan has split rows (a finalize pass)" :
                      (a.epi_op != LLMREC_SPMM_EPI_NONE || a.post_scale) ? "an epilogue (softmax or post_scale)" :
                      (!weighted && a.Z) ? "an init term on the unweighted product" :
                      (a.y_needed || a.listed_only) ? "a row restriction" : nullptr;
    if (why) {
        set_error("spmm (hosted): compiled for the whole-row product, plain without an epilogue or weighted by col_scale with an init term: %s", why);
        return LLMREC_EUNSUPPORTED;
    }
    out.a = a;
    out.weighted = weighted;
    out.blocks = spmm_layout(out.a, kSpmmFamilyLpr[pp.family], 0, tpb);
    if (out.blocks < 0) { set_error("spmm (hosted): too many rows for one launch"); return LLMREC_EUNSUPPORTED; }
    out.bytes_x = pp.bytes_x; out.bytes_y = pp.bytes_y; out.bytes_z = pp.bytes_z;
    return LLMREC_OK;
}

// One unmasked product for a launch of its own by another translation unit (spmm_body.h: SpmmSingle; the caller has refused the masks).
int spmm_prepare_single(const llmrec_spmm_problem_t& pr, SpmmSingle& out) {
    SpmmPrepared pp;
    const int rc = spmm_prepare(pr, pp);
    if (rc != LLMREC_OK) return rc;
    out.a = pp.a; out.family = pp.family; out.weighted = pp.variant == SPMM_V_WEIGHTED || pp.variant == SPMM_V_MASKED_W;
    out.empty = pp.empty; out.blocks = 0;
    if (pp.empty) return LLMREC_OK;
    out.blocks = spmm_layout(out.a, kSpmmFamilyLpr[pp.family], 0);
    if (out.blocks < 0) { set_error("spmm: too many rows for one launch"); return LLMREC_EUNSUPPORTED; }
    return LLMREC_OK;
}

// Checks every problem, lays the non-empty ones out back to back (in the caller's order) and launches them together.
static int spmm_run(int32_t n, const llmrec_spmm_problem_t* problems, hipStream_t stream, const llmrec_spmm_guest_t* guest = nullptr) {
    LLMREC_CHECK_ARG(n >= 0 && n <= LLMREC_SPMM_MAX_PROBLEMS && (n == 0 || problems), "spmm_multi: n = %d outside 0..%d", n, LLMREC_SPMM_MAX_PROBLEMS);
    SpmmPrepared pp[LLMREC_SPMM_MAX_PROBLEMS];
    int m = 0;
    for (int q = 0; q < n; ++q) {
        const int rc = spmm_prepare(problems[q], pp[m]);
        if (rc != LLMREC_OK) return rc;
        if (!pp[m].empty) ++m;
    }
    // a slice-masked product takes along the members of its group that its instance can run - the same family, weighted by col_scale
    // alone (rows_body_pipe_smask reads no val) and without y_row_needed (it computes every row): they run with a mask that begins
    // behind their last slice (a no-op). Any other company keeps its variant and is refused below like any mixed group
    bool smask = false;
    for (int q = 0; q < m; ++q) smask = smask || pp[q].variant == SPMM_V_SMASK_W;
    for (int q = 0; q < m && smask; ++q) {
        const SpmmArgs& aq = pp[q].a;
        if (pp[q].variant != SPMM_V_WEIGHTED || pp[q].family != 2 || aq.val || !aq.col_scale || aq.y_needed) continue;
        pp[q].variant = SPMM_V_SMASK_W;
        pp[q].a.smask_col0 = pp[q].a.n_slices * pp[q].a.d;
    }
    GuestLaunch gl = {};
    if (guest) {                                                         // every check of the guest too, before anything is launched
        int rc;
        gl.kind = guest->kind;
        if (guest->kind == LLMREC_SPMM_GUEST_SAMPLER) rc = guest_prepare(guest->u.sampler, TPB, "spmm_multi_guest (sampler)", gl.sampler, gl.blocks, gl.shmem);
        else if (guest->kind == LLMREC_SPMM_GUEST_PLAN_REACH) rc = guest_prepare(guest->u.plan_reach, TPB, "spmm_multi_guest (plan + reach marks)", gl.plan_reach, gl.blocks, gl.shmem);
        else if (guest->kind == LLMREC_SPMM_GUEST_LOSSES) rc = guest_prepare(guest->u.losses, TPB, "spmm_multi_guest (loss values)", gl.losses, gl.blocks, gl.shmem);
        else { set_error("spmm_multi_guest: unknown guest kind %d", guest->kind); return LLMREC_EINVAL; }
        if (rc != LLMREC_OK) return rc;
        if (gl.blocks == 0 || m == 0) {
            set_error("spmm_multi_guest: an empty guest or no non-empty problem to host it");
            return LLMREC_EUNSUPPORTED;
        }
        // the plan's keys are dynamic LDS of EVERY block of the launch: three 512-thread blocks (7 waves/SIMD) must still fit a CU's 160 KB
        if (guest->kind == LLMREC_SPMM_GUEST_PLAN_REACH && guest->u.plan_reach.B_max > LLMREC_SPMM_GUEST_MAX_PLAN_B) {
            set_error("spmm_multi_guest: a plan of B_max %d > %d would cost the launch its occupancy", guest->u.plan_reach.B_max, LLMREC_SPMM_GUEST_MAX_PLAN_B);
            return LLMREC_EUNSUPPORTED;
        }
        if (smask && guest->kind != LLMREC_SPMM_GUEST_LOSSES) {
            set_error("spmm_multi_guest: the slice-masked product hosts the loss values only (guest kind %d)", guest->kind);
            return LLMREC_EUNSUPPORTED;
        }
        if (!(pp[0].family == 2 && (pp[0].variant == SPMM_V_PLAIN || pp[0].variant == SPMM_V_WEIGHTED || pp[0].variant == SPMM_V_SMASK_W))) {
            set_error("spmm_multi_guest: compiled for the unmasked float4 products of 33..64 columns only (family %d, variant %d)", pp[0].family, pp[0].variant);
            return LLMREC_EUNSUPPORTED;
        }
    }
    if (m == 0) return LLMREC_OK;
    for (int q = 1; q < m; ++q) {
        if (pp[q].family != pp[0].family || pp[q].variant != pp[0].variant) {
            set_error("spmm_multi: problem %d resolves to another kernel instance than problem 0 (family %d / %d, variant %d / %d)",
                      q, pp[q].family, pp[0].family, pp[q].variant, pp[0].variant);
            return LLMREC_EUNSUPPORTED;
        }
    }
    if (m > 1 && !(pp[0].family <= 6 && (pp[0].variant == SPMM_V_PLAIN || pp[0].variant == SPMM_V_WEIGHTED || pp[0].variant == SPMM_V_SMASK_W))) {
        set_error("spmm_multi: grouped launches are compiled for the unmasked products with vector loads only");
        return LLMREC_EUNSUPPORTED;
    }
    // what one problem writes (Y, its partials) must not be read or written by another one: they run concurrently
    for (int i = 0; i < m; ++i) {
        for (int j = 0; j < m; ++j) {
            if (i == j) continue;
            const SpmmArgs &ai = pp[i].a, &aj = pp[j].a;
            const void* wr[2] = {ai.Y, ai.partials};
            const int64_t wn[2] = {pp[i].bytes_y, pp[i].bytes_partials};
            const void* rd[5] = {aj.X, aj.Y, aj.Z, aj.S, aj.partials};
            const int64_t rn[5] = {pp[j].bytes_x, pp[j].bytes_y, pp[j].bytes_z, pp[j].bytes_s, pp[j].bytes_partials};
            for (int u = 0; u < 2; ++u)
                for (int v = 0; v < 5; ++v)
                    LLMREC_CHECK_ARG(!bytes_overlap(wr[u], wn[u], rd[v], rn[v]), "spmm_multi: the output of problem %d overlaps an operand of problem %d", i, j);
        }
    }
    const int lpr = kSpmmFamilyLpr[pp[0].family];
    int64_t total = gl.blocks;                                           // (0 without a guest: its blocks come first)
    for (int q = 0; q < m; ++q) {
        const int64_t t = spmm_layout(pp[q].a, lpr, total);
        if (t < 0) { set_error("spmm: too many rows for one launch"); return LLMREC_EUNSUPPORTED; }
        total += t;
    }
    const int v = pp[0].variant;
    switch (pp[0].family) {
    case 0: return launch_spmm<4, 1, 4>(m, pp, v, total, stream);
    case 1: return launch_spmm<8, 1, 4>(m, pp, v, total, stream);
    case 2: return launch_spmm<16, 1, 4>(m, pp, v, total, stream, guest ? &gl : nullptr);
    case 3: return launch_spmm<32, 1, 4>(m, pp, v, total, stream);
    case 4: return launch_spmm<64, 1, 4>(m, pp, v, total, stream);
    case 5: return launch_spmm<64, 2, 4>(m, pp, v, total, stream);
    case 6: return launch_spmm<64, 4, 4>(m, pp, v, total, stream);
    case 7: return launch_spmm<16, 1, 1>(m, pp, v, total, stream);
    case 8: return launch_spmm<64, 1, 1>(m, pp, v, total, stream);
    default: return launch_spmm<64, 4, 1>(m, pp, v, total, stream);
    }
}

}  // namespace llmrec

using namespace llmrec;

extern "C" int llmrec_spmm_f32(int64_t n_rows, int64_t n_cols,
                               const int32_t* rowptr, const int32_t* colidx, const float* val,
                               const float* row_scale, const float* col_scale,
                               const float* X, int64_t ldx, float* Y, int64_t ldy, int32_t d, int32_t slice_width,
                               const llmrec_spmm_plan_t* plan_host, float* partials,
                               const llmrec_spmm_epilogue_t* epilogue_host, llmrec_stream_t stream_) {
    llmrec_spmm_problem_t pr = {n_rows, n_cols, rowptr, colidx, val, row_scale, col_scale, X, ldx, Y, ldy, d, slice_width,
                                plan_host, partials, epilogue_host};
    return spmm_run(1, &pr, (hipStream_t)stream_);
}

extern "C" int llmrec_spmm_multi_f32(int32_t n, const llmrec_spmm_problem_t* problems, llmrec_stream_t stream_) {
    return spmm_run(n, problems, (hipStream_t)stream_);
}

extern "C" int llmrec_spmm_multi_guest_f32(int32_t n, const llmrec_spmm_problem_t* problems, const llmrec_spmm_guest_t* guest, llmrec_stream_t stream_) {
    LLMREC_CHECK_ARG(guest, "spmm_multi_guest: no guest (llmrec_spmm_multi_f32 is the call without one)");
    return spmm_run(n, problems, (hipStream_t)stream_, guest);
}

extern "C" int64_t llmrec_spmm_rows_compact_workspace_bytes(int64_t capacity, int32_t d) {
    if (capacity < 0 || d <= 0) return -1;
    return align_up(capacity * LLMREC_SPMM_COMPACT_PARTS * (int64_t)d * 4, 256);
}

extern "C" int llmrec_spmm_rows_compact_f32(int64_t n_rows, int64_t n_cols, const int32_t* rowptr, const int32_t* colidx, const float* row_scale,
                                            const float* X, int64_t ldx, int32_t d, const int32_t* row_list, const int32_t* n_list_dev,
                                            int32_t capacity, float* out, int64_t ldo, void* workspace, int64_t workspace_bytes,
                                            llmrec_stream_t stream_) {
    LLMREC_CHECK_ARG(n_rows >= 0 && n_cols >= 0 && d > 0 && capacity >= 0, "spmm_rows_compact: bad sizes");
    if (capacity == 0) return LLMREC_OK;
    LLMREC_CHECK_ARG(rowptr && colidx && X && row_list && n_list_dev && out && ldx >= d && ldo >= d, "spmm_rows_compact: null pointer or ld < d");
    LLMREC_CHECK_ARG(capacity <= 65535 * 16, "spmm_rows_compact: capacity too large for one launch");
    if (!workspace || workspace_bytes < llmrec_spmm_rows_compact_workspace_bytes(capacity, d)) {
        set_error("spmm_rows_compact: workspace %lld < %lld", (long long)workspace_bytes, (long long)llmrec_spmm_rows_compact_workspace_bytes(capacity, d));
        return LLMREC_EWORKSPACE;
    }
    SpmmArgs a = {};
    a.n_rows = n_rows; a.rowptr = rowptr; a.colidx = colidx; a.row_scale = row_scale; a.X = X; a.ldx = ldx; a.d = d; a.n_slices = 1;
    hipStream_t stream = (hipStream_t)stream_;
    float* partial = (float*)workspace;
    const bool vec4 = (d % 4 == 0) && (ldx % 4 == 0) && (ldo % 4 == 0) && (((uintptr_t)X | (uintptr_t)out | (uintptr_t)partial) % 16 == 0);
    if (vec4) {
        if (d <= 16) return launch_rows_compact<4, 1, 4>(a, row_list, n_list_dev, capacity, out, ldo, partial, stream);
        if (d <= 32) return launch_rows_compact<8, 1, 4>(a, row_list, n_list_dev, capacity, out, ldo, partial, stream);
        if (d <= 64) return launch_rows_compact<16, 1, 4>(a, row_list, n_list_dev, capacity, out, ldo, partial, stream);
        if (d <= 128) return launch_rows_compact<32, 1, 4>(a, row_list, n_list_dev, capacity, out, ldo, partial, stream);
        if (d <= 256) return launch_rows_compact<64, 1, 4>(a, row_list, n_list_dev, capacity, out, ldo, partial, stream);
    } else {
        if (d <= 16) return launch_rows_compact<16, 1, 1>(a, row_list, n_list_dev, capacity, out, ldo, partial, stream);
        if (d <= 64) return launch_rows_compact<64, 1, 1>(a, row_list, n_list_dev, capacity, out, ldo, partial, stream);
    }
    set_error("spmm_rows_compact: d = %d outside the compiled kernel family (vec4 = %d)", d, (int)vec4);
    return LLMREC_EUNSUPPORTED;
}
