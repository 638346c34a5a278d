// spmm_body.h - the device side of the SpMM (spmm.hip: organisation, buckets, summation trees): the argument block and the bodies of one
// block of a product. Shared by the SpMM launches (spmm.hip) and by the launch of another kernel that hosts a product as extra blocks
// (dense.hip: the grouped projection). The bodies that a host runs take their block size as the template parameter BT; every
// summation tree is that of the 512-thread launch whatever BT is.
#pragma once
#include "common.h"

namespace llmrec {

constexpr int UNROLL = 8;

template <int VEC> struct Vec;
template <> struct Vec<4> {
    float4 v;
    __device__ __forceinline__ void zero() { v = make_float4(0.f, 0.f, 0.f, 0.f); }
    __device__ __forceinline__ void load(const float* p) { v = *reinterpret_cast<const float4*>(p); }
    __device__ __forceinline__ void store(float* p) const { *reinterpret_cast<float4*>(p) = v; }
    // four bf16 values (one 8-byte access), widened exactly: a bf16 is the high half of the fp32 with the same value
    __device__ __forceinline__ void load(const uint16_t* p) {
        const uint2 r = *reinterpret_cast<const uint2*>(p);
        v = make_float4(__uint_as_float(r.x << 16), __uint_as_float(r.x & 0xffff0000u), __uint_as_float(r.y << 16), __uint_as_float(r.y & 0xffff0000u));
    }
    __device__ __forceinline__ void store_bf16(uint16_t* p) const {
        *reinterpret_cast<uint2*>(p) = make_uint2(rn_bf16_bits(v.x) >> 16 | rn_bf16_bits(v.y), rn_bf16_bits(v.z) >> 16 | rn_bf16_bits(v.w));
    }
    __device__ __forceinline__ void add(const Vec& o) { v.x += o.v.x; v.y += o.v.y; v.z += o.v.z; v.w += o.v.w; }
    __device__ __forceinline__ void fma(float w, const Vec& o) {
        v.x = fmaf(w, o.v.x, v.x); v.y = fmaf(w, o.v.y, v.y); v.z = fmaf(w, o.v.z, v.z); v.w = fmaf(w, o.v.w, v.w);
    }
    __device__ __forceinline__ void scale(float s) { v.x *= s; v.y *= s; v.z *= s; v.w *= s; }
    __device__ __forceinline__ void xor_add(int off) {
        v.x += __shfl_xor(v.x, off, 64); v.y += __shfl_xor(v.y, off, 64);
        v.z += __shfl_xor(v.z, off, 64); v.w += __shfl_xor(v.w, off, 64);
    }
    __device__ __forceinline__ float hmax() const { return fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)); }
    __device__ __forceinline__ float hsum() const { return (v.x + v.y) + (v.z + v.w); }
    // (x0 y0 + x1 y1) + (x2 y2 + x3 y3) with its two fused multiply-adds WRITTEN OUT and no contraction left to the compiler: how the
    // plain expression is contracted depends on the code around it, and the softmax backward of one row must round the same way in
    // every kernel that finishes it (the fp32 and the bf16-row products, single and grouped launches: they are compared bit for bit)
    __device__ __forceinline__ float dot(const Vec& o) const {
#pragma clang fp contract(off)
        const float t1 = __builtin_fmaf(v.x, o.v.x, v.y * o.v.y), t2 = __builtin_fmaf(v.z, o.v.z, v.w * o.v.w);
        return t1 + t2;
    }
    __device__ __forceinline__ void exp_sub(float m) { v.x = expf(v.x - m); v.y = expf(v.y - m); v.z = expf(v.z - m); v.w = expf(v.w - m); }
    // this = s * (this - c)    (softmax backward: y * (g - sum(g y)))
    __device__ __forceinline__ void sub_mul(float c, const Vec& s) { v.x = s.v.x * (v.x - c); v.y = s.v.y * (v.y - c); v.z = s.v.z * (v.z - c); v.w = s.v.w * (v.w - c); }
};
template <> struct Vec<1> {
    float v;
    __device__ __forceinline__ void zero() { v = 0.f; }
    __device__ __forceinline__ void load(const float* p) { v = *p; }
    __device__ __forceinline__ void store(float* p) const { *p = v; }
    __device__ __forceinline__ void add(const Vec& o) { v += o.v; }
    __device__ __forceinline__ void fma(float w, const Vec& o) { v = fmaf(w, o.v, v); }
    __device__ __forceinline__ void scale(float s) { v *= s; }
    __device__ __forceinline__ void xor_add(int off) { v += __shfl_xor(v, off, 64); }
    __device__ __forceinline__ float hmax() const { return v; }
    __device__ __forceinline__ float hsum() const { return v; }
    __device__ __forceinline__ float dot(const Vec& o) const { return v * o.v; }
    __device__ __forceinline__ void exp_sub(float m) { v = expf(v - m); }
    __device__ __forceinline__ void sub_mul(float c, const Vec& s) { v = s.v * (v - c); }
};

struct SpmmArgs {
    int64_t n_rows;
    const int32_t* rowptr;
    const int32_t* colidx;
    const float* val;
    const float* row_scale;
    const float* col_scale;
    const float* X;
    int64_t ldx;
    float* Y;
    int64_t ldy;
    int32_t d;                   // columns handled per task (= the slice width when the operand is cut into column slices)
    int32_t n_slices;            // column slices of width d: task (row, slice) reads / writes columns [slice d, (slice + 1) d)
    // epilogue: t = alpha * Z[row] + result; Y[row] = op(t)
    int32_t epi_op;
    float alpha;
    const float* Z;
    int64_t ldz;
    const float* S;              // softmax backward: rows of the forward softmax output
    int64_t lds;
    const float* post_scale;     // per-row scale of the output, applied last
    // operand sparsity (llmrec_spmm_epilogue_t): X rows whose byte in x_mask differs from x_active are all-zero and are not read;
    // y_flag[row] := x_active if the row's result can be non-zero (an active X row was gathered, or z_flag[row] == x_active), else 0
    const uint8_t* x_mask;
    int32_t x_active;
    uint8_t* y_flag;
    const uint8_t* z_flag;
    const uint8_t* y_gate;       // rows whose byte != x_active: no active neighbour, zero Z row - written as zeros at once
    const uint8_t* y_needed;     // rows whose byte != x_active are neither computed nor written (short-row range)
    int32_t listed_only;         // no short-row range at all: only the plan's row lists are computed
    int32_t pipe;                // > 1: tasks per lane group of the short-row range, run as a software pipeline (rows_body_pipe)
    // slice-ranged mask with a device stamp (llmrec_spmm_epilogue_t.x_mask_stamp; the SMASK kernels only): in tasks whose first column is
    // >= smask_col0, X rows whose smask byte differs from LLMREC_ROW_STAMP(*smask_stamp) are all-zero and are not read. smask NULL and
    // smask_col0 = n_slices * d: a member of a grouped launch without a mask of its own
    const uint8_t* smask;
    const int32_t* smask_stamp;
    int32_t smask_col0;
    int32_t smask_inplace;       // Y += A X in place (Z = Y, alpha 1, no op, no post_scale): a masked task without an active neighbour leaves its row alone
    // plan
    const int32_t* slot_row;     // non-NULL: rowptr / colidx are the PERMUTED CSR of the plan - CSR row `slot` is output row slot_row[slot], the
    int32_t n_short_rows;        // first n_short_rows slots are the lane-group bucket, the plan's lists hold slots (llmrec_spmm_plan_t)
    const int32_t* wave_rows;
    const int32_t* block_rows;
    const int32_t* split_rows;
    const int32_t* split_seg_begin;
    const int32_t* seg_split;
    float* partials;             // [slice][segment][d]
    int32_t n_wave_rows, n_block_rows, n_split_rows, n_segments, segment;
    // block ranges of the launch (global block ids: a grouped launch, llmrec_spmm_multi_f32, gives each problem a range of its own):
    // [blk_begin, blk_seg) segments of the split rows, [blk_seg, blk_block) block rows, [blk_block, blk_wave) wave rows,
    // [blk_wave, blk_end) short rows
    int32_t blk_begin, blk_seg, blk_block, blk_wave, blk_end;
};

// The product that gathers BF16 rows (spmm_bf16.hip: llmrec_spmm_xbf16_f32). The bodies below take their argument block as a template
// parameter and reach the gathered operand and the finished row through x_row / store_shadow only: with SpmmArgs they are the fp32
// product, token for token; with SpmmArgsXb every gather is one 8-byte load of four bf16 values widened by a shift (Vec<4>::load) - the
// same lanes, chunks and order of additions, so the result is bit for bit that of the fp32 product on the widened operand - and the
// finished row (after the epilogue and post_scale) is also stored rounded to bf16 when Yb is given.
struct SpmmArgsXb : SpmmArgs {
    const uint16_t* Xb;          // [n_cols, d] bf16 rows (SpmmArgs::X is unused)
    int64_t ldxb;
    uint16_t* Yb;                // NULL, or [n_rows, d]: Yb[r] = RNE_bf16(Y[r])
    int64_t ldyb;
};
__device__ __forceinline__ const float* x_row(const SpmmArgs& a, int32_t c) { return a.X + (int64_t)c * a.ldx; }
__device__ __forceinline__ const uint16_t* x_row(const SpmmArgsXb& a, int32_t c) { return a.Xb + (int64_t)c * a.ldxb; }
template <int VEC> __device__ __forceinline__ void store_shadow(const SpmmArgs&, int64_t, int64_t, const Vec<VEC>&) {}
__device__ __forceinline__ void store_shadow(const SpmmArgsXb& a, int64_t row, int64_t col, const Vec<4>& v) {
    if (a.Yb) v.store_bf16(a.Yb + row * a.ldyb + col);
}

// Accumulate sum_{j in [s, e)} w_j * X[col_j, chunk columns] into acc, in ascending j order. MASKED: rows of X that are not active
// (a.x_mask) are known to be all-zero and are not fetched; `any` collects whether this lane saw an active column.
// unmasked ranges (round 6): the NEXT chunk's column indices (and adjacency values) are fetched while the current chunk's rows are gathered, the
// col_scale factors of the current chunk ride beside its gathers - one memory round trip per chunk of LPR non-zeros instead of two or three.
// Same gathers, same order of additions as one chunk at a time: bit-identical to the masked loop with every column active.
template <int LPR, int NCHUNK, int VEC, bool WEIGHTED, class A>
__device__ __forceinline__ void accumulate_range_plain(const A& a, int64_t col0, int32_t s, int32_t e, int gl, Vec<VEC> (&acc)[NCHUNK]) {
    int32_t c_next = 0;
    float v_next = 1.0f;
    if (s + gl < e) { c_next = a.colidx[s + gl]; if (WEIGHTED && a.val) v_next = a.val[s + gl]; }
    for (int32_t base = s; base < e; base += LPR) {
        const int n = min(LPR, e - base);
        const int32_t myc = c_next;
        float myw = v_next;
        const int32_t nb = base + LPR;
        if (nb + gl < e) { c_next = a.colidx[nb + gl]; if (WEIGHTED && a.val) v_next = a.val[nb + gl]; }
        float cs = 1.0f;
        if (WEIGHTED && a.col_scale && gl < n) cs = a.col_scale[myc];        // (in flight beside the gathers below)
        for (int t = 0; t < n; t += UNROLL) {
            Vec<VEC> v[UNROLL][NCHUNK];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                const int tt = t + u;
                const int32_t c = __shfl(myc, tt & (LPR - 1), LPR);
                const auto* xr = x_row(a, c) + col0;
#pragma unroll
                for (int k = 0; k < NCHUNK; ++k) {
                    const int col = (k * LPR + gl) * VEC;
                    if (tt < n && col < a.d) v[u][k].load(xr + col);
                    else v[u][k].zero();
                }
            }
            if (WEIGHTED && t == 0) myw = gl < n ? myw * cs : 0.f;            // val[e] * col_scale[c], as the masked loop forms it
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                float w = 0.f;
                if (WEIGHTED) w = __shfl(myw, (t + u) & (LPR - 1), LPR);
#pragma unroll
                for (int k = 0; k < NCHUNK; ++k) {
                    if (WEIGHTED) acc[k].fma(w, v[u][k]);
                    else acc[k].add(v[u][k]);
                }
            }
        }
    }
}

template <int LPR, int NCHUNK, int VEC, bool WEIGHTED, bool MASKED, class A>
__device__ __forceinline__ void accumulate_range(const A& a, int64_t col0, int32_t s, int32_t e, int gl, Vec<VEC> (&acc)[NCHUNK], int& any,
                                                 const uint8_t* xm, int xa) {
    if constexpr (!MASKED) {
        accumulate_range_plain<LPR, NCHUNK, VEC, WEIGHTED>(a, col0, s, e, gl, acc);
    } else {
        for (int32_t base = s; base < e; base += LPR) {
            const int n = min(LPR, e - base);
            int32_t myc = 0;
            float myw = 0.f;
            int myact = 0;
            if (gl < n) {
                myc = a.colidx[base + gl];
                if (WEIGHTED) {
                    myw = a.val ? a.val[base + gl] : 1.0f;
                    if (a.col_scale) myw *= a.col_scale[myc];
                }
                myact = (int)xm[myc] == xa; any |= myact;
            }
            // only the ACTIVE columns of this chunk are visited (ascending, as in the dense loop: the skipped terms are exact zeros)
            const unsigned long long bal = __ballot(myact != 0);
            const int g0 = (int)(threadIdx.x & 63) / LPR * LPR;
            unsigned long long bits = LPR >= 64 ? bal : ((bal >> g0) & ((1ull << LPR) - 1ull));      // uniform per lane group
            while (bits) {
                Vec<VEC> v[UNROLL][NCHUNK];
                float w[UNROLL];
#pragma unroll
                for (int u = 0; u < UNROLL; ++u) {
                    const bool valid = bits != 0ull;
                    const int j = valid ? __builtin_ctzll(bits) : 0;
                    bits &= bits - 1ull;                                   // (0 stays 0)
                    const int32_t c = __shfl(myc, j, LPR);
                    if (WEIGHTED) w[u] = valid ? __shfl(myw, j, LPR) : 0.f; else w[u] = 0.f;
                    const auto* xr = x_row(a, c) + col0;
#pragma unroll
                    for (int k = 0; k < NCHUNK; ++k) {
                        const int col = (k * LPR + gl) * VEC;
                        if (valid && col < a.d) v[u][k].load(xr + col);
                        else v[u][k].zero();
                    }
                }
#pragma unroll
                for (int u = 0; u < UNROLL; ++u) {
#pragma unroll
                    for (int k = 0; k < NCHUNK; ++k) {
                        if (WEIGHTED) acc[k].fma(w[u], v[u][k]);
                        else acc[k].add(v[u][k]);
                    }
                }
            }
        }
    }
}

// the output-row flag of a masked product (see SpmmArgs); returns whether the row is known to be all-zero AND may be written as
// zeros without its epilogue (Z absent or known zero through z_flag; the forward softmax of a zero row is not zero)
__device__ __forceinline__ bool write_row_flag(const SpmmArgs& a, int64_t row, bool any_active, bool write) {
    const bool z = a.z_flag && (int)a.z_flag[row] == a.x_active;
    if (write && a.y_flag) a.y_flag[row] = (any_active || z) ? (uint8_t)a.x_active : (uint8_t)0;
    return !any_active && !z && (a.Z == nullptr || a.z_flag != nullptr) && a.epi_op != LLMREC_SPMM_EPI_SOFTMAX;
}

// The finished row (unscaled sum in acc, held by the LPR lanes of one lane group): scale, init term, epilogue, store.
template <int LPR, int NCHUNK, int VEC, class A>
__device__ __forceinline__ void finish_row(const A& a, int64_t col0, int64_t row, int gl, Vec<VEC> (&acc)[NCHUNK], bool zero_row = false) {
    const float rs = a.row_scale ? a.row_scale[row] : 1.0f;
    float* yr = a.Y + row * a.ldy + col0;
    if (zero_row) {                                              // (uniform per lane group) a masked product's row without an active neighbour
#pragma unroll                                                   // and with an unflagged (= zero) Z row: op(0) = 0 for op in {none, softmax
        for (int k = 0; k < NCHUNK; ++k) {                       // backward} - written without reading Z / S
            const int col = (k * LPR + gl) * VEC;
            acc[k].zero();
            if (col < a.d) acc[k].store(yr + col);
        }
        return;
    }
#pragma unroll
    for (int k = 0; k < NCHUNK; ++k) {
        const int col = (k * LPR + gl) * VEC;
        if (a.row_scale) acc[k].scale(rs);
        if (a.Z && col < a.d) { Vec<VEC> z; z.load(a.Z + row * a.ldz + col0 + col); acc[k].fma(a.alpha, z); }
        if (col >= a.d) acc[k].zero();
    }
    if (a.epi_op == LLMREC_SPMM_EPI_SOFTMAX) {                   // wave-uniform
        float m = -INFINITY;
#pragma unroll
        for (int k = 0; k < NCHUNK; ++k) if ((k * LPR + gl) * VEC < a.d) m = fmaxf(m, acc[k].hmax());
        m = group_max<LPR>(m);
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < NCHUNK; ++k) {
            if ((k * LPR + gl) * VEC < a.d) { acc[k].exp_sub(m); s += acc[k].hsum(); }
        }
        s = group_sum<LPR>(s);
        const float inv = 1.0f / s;
#pragma unroll
        for (int k = 0; k < NCHUNK; ++k) acc[k].scale(inv);
    } else if (a.epi_op == LLMREC_SPMM_EPI_SOFTMAX_BWD) {
        Vec<VEC> y[NCHUNK];
        float c = 0.f;
#pragma unroll
        for (int k = 0; k < NCHUNK; ++k) {
            const int col = (k * LPR + gl) * VEC;
            if (col < a.d) { y[k].load(a.S + row * a.lds + col0 + col); c += acc[k].dot(y[k]); }
            else y[k].zero();
        }
        c = group_sum<LPR>(c);
#pragma unroll
        for (int k = 0; k < NCHUNK; ++k) acc[k].sub_mul(c, y[k]);
    }
    if (a.post_scale) {
        const float ps = a.post_scale[row];
#pragma unroll
        for (int k = 0; k < NCHUNK; ++k) acc[k].scale(ps);
    }
#pragma unroll
    for (int k = 0; k < NCHUNK; ++k) {
        const int col = (k * LPR + gl) * VEC;
        if (col < a.d) { acc[k].store(yr + col); store_shadow(a, row, col0 + col, acc[k]); }
    }
}

constexpr int TPB = 512;                                        // threads per block: 8 wavefronts

// one lane group per (row, slice) task; rows with more than LLMREC_SPMM_LONG_ROW nnz belong to the other ranges
template <int LPR, int NCHUNK, int VEC, bool WEIGHTED, bool MASKED, int BT = TPB, class A>
__device__ __forceinline__ void rows_body(const A& a, int64_t block) {
    constexpr int GPB = BT / LPR;
    const int gl = threadIdx.x & (LPR - 1);
    const int64_t task = block * GPB + (threadIdx.x / LPR);
    const int64_t n_list = a.slot_row ? (int64_t)a.n_short_rows : a.n_rows;
    if (task >= n_list * a.n_slices) return;
    const int64_t slice = task / n_list, slot = task - slice * n_list;         // slice-major: neighbouring lane groups take neighbouring rows
    const int64_t row = a.slot_row ? (int64_t)a.slot_row[slot] : slot;         // (permuted CSR: by descending length class - equal lengths side by side)
    const int64_t col0 = slice * a.d;
    if (a.y_needed && (int)a.y_needed[row] != a.x_active) return;                // (uniform per lane group) nobody reads this row
    const int32_t s = a.rowptr[slot], e = a.rowptr[slot + 1];
    if (!a.slot_row && (e - s) > LLMREC_SPMM_LONG_ROW) return;
    Vec<VEC> acc[NCHUNK];
#pragma unroll
    for (int k = 0; k < NCHUNK; ++k) acc[k].zero();
    int any = 0;
    bool zero_row = false;
    if (MASKED && a.y_gate && (int)a.y_gate[row] != a.x_active) {         // (uniform per lane group) gated out: nothing of the row is read
        if (a.y_flag && slice == 0 && gl == 0) a.y_flag[row] = 0;
        finish_row<LPR, NCHUNK, VEC>(a, col0, row, gl, acc, true);
        return;
    }
    if (MASKED) {
        // most rows of a masked product have no active neighbour at all: look at the index list and the mask bytes first (two dependent
        // loads, no per-edge arithmetic) and leave at once when nothing is active - the accumulation loop runs for the few other rows only
        for (int32_t base = s; base < e; base += LPR)
            if (base + gl < e) any |= (int)a.x_mask[a.colidx[base + gl]] == a.x_active;
        const unsigned long long bal = __ballot(any != 0);                // (uniform per lane group below)
        const int g0 = (int)(threadIdx.x & 63) / LPR * LPR;
        const unsigned long long gm = LPR >= 64 ? ~0ull : (((1ull << LPR) - 1ull) << g0);
        const bool any_g = (bal & gm) != 0ull;
        zero_row = write_row_flag(a, row, any_g, slice == 0 && gl == 0);
        if (any_g) accumulate_range<LPR, NCHUNK, VEC, WEIGHTED, MASKED>(a, col0, s, e, gl, acc, any, a.x_mask, a.x_active);
    } else {
        accumulate_range<LPR, NCHUNK, VEC, WEIGHTED, MASKED>(a, col0, s, e, gl, acc, any, a.x_mask, a.x_active);
    }
    finish_row<LPR, NCHUNK, VEC>(a, col0, row, gl, acc, zero_row);
}

// PIPELINED short rows (round 6). A (row, slice) task of the lane-group bucket is three DEPENDENT memory round trips - {slot -> output row,
// row pointers} -> column indices -> X rows - for a handful of gathers, and a launch-bound product (the step's [rows, 7 x 64] side products:
// 121 k tasks, ~32 k lane groups resident) pays them once per round of resident blocks: 4 rounds x 3 latencies. Here a lane group takes
// `pipe` tasks (task, task + G, task + 2 G, ...: neighbouring groups keep neighbouring slots) and runs them as a software pipeline: while the
// rows of task i are gathered, the indices of task i + 1 and the row pointers of task i + 2 are already in flight - ONE round trip per task
// after a two-deep prologue, and pipe x fewer blocks to schedule. Same gathers in the same order: bit-identical sums. (The other shape tried -
// one task per row looping over the slices, indices loaded once - was no faster in the step and slower alone: 29.4 vs 28.3 us.)
template <int LPR, int NCHUNK, int VEC, bool WEIGHTED, int BT = TPB, class A>
__device__ __forceinline__ void rows_body_pipe(const A& a, int64_t block, int64_t n_blocks) {
    constexpr int GPB = BT / LPR;
    constexpr int NI = (LLMREC_SPMM_LONG_ROW + LPR - 1) / LPR;         // index registers per lane
    const int gl = threadIdx.x & (LPR - 1);
    // (32-bit task arithmetic: the host enables the pipeline only below 2^31 tasks - fewer registers, no 64-bit divisions)
    const int32_t n_list = (int32_t)(a.slot_row ? (int64_t)a.n_short_rows : a.n_rows);
    const int32_t n_tasks = n_list * a.n_slices, G = (int32_t)n_blocks * GPB;
    int32_t t0 = (int32_t)block * GPB + (int32_t)(threadIdx.x / LPR);
    if (t0 >= n_tasks) return;
    auto level1 = [&](int32_t t, int32_t& row, int32_t& s_, int32_t& n_, int32_t& col0) {    // slot -> output row, row pointers (independent loads)
        const int32_t slice = t / n_list, slot = t - slice * n_list;
        row = a.slot_row ? a.slot_row[slot] : slot;
        s_ = a.rowptr[slot]; n_ = a.rowptr[slot + 1] - s_;
        col0 = slice * a.d;
    };
    auto level2 = [&](int32_t s_, int32_t n_, int32_t (&c)[NI]) {                              // the row's column indices (<= LONG_ROW of them)
#pragma unroll
        for (int k = 0; k < NI; ++k) { const int j = k * LPR + gl; c[k] = (j < n_ && n_ <= LLMREC_SPMM_LONG_ROW) ? a.colidx[s_ + j] : 0; }
    };
    int32_t row0, col00, row1 = 0, col01 = 0;
    int32_t s0, n0, s1 = 0, n1 = 0, c0[NI], c1[NI];
    level1(t0, row0, s0, n0, col00);
    level2(s0, n0, c0);
    int32_t t1 = t0 + G;
    bool has1 = t1 < n_tasks;
    if (has1) level1(t1, row1, s1, n1, col01);
    for (;;) {
        int32_t row2 = 0, col02 = 0;
        int32_t s2 = 0, n2 = 0;
        const int32_t t2 = t1 + G;
        const bool has2 = has1 && t2 < n_tasks;
        if (has1) level2(s1, n1, c1);                                   // in flight while task 0's rows are gathered
        if (has2) level1(t2, row2, s2, n2, col02);
        if (n0 <= LLMREC_SPMM_LONG_ROW && !(a.y_needed && (int)a.y_needed[row0] != a.x_active)) {   // (longer: a row of another bucket, plain plans only)
            float w0[NI];
            if (WEIGHTED) {
#pragma unroll
                for (int k = 0; k < NI; ++k) {
                    const int j = k * LPR + gl;
                    w0[k] = 0.f;
                    if (j < n0) { w0[k] = a.val ? a.val[s0 + j] : 1.0f; if (a.col_scale) w0[k] *= a.col_scale[c0[k]]; }
                }
            }
            Vec<VEC> acc[NCHUNK];
#pragma unroll
            for (int k = 0; k < NCHUNK; ++k) acc[k].zero();
#pragma unroll
            for (int ki = 0; ki < NI; ++ki) {
                const int nk = min(LPR, n0 - ki * LPR);                 // indices of this register that are in the row (uniform per lane group)
                for (int t = 0; t < nk; t += UNROLL) {
                    Vec<VEC> v[UNROLL][NCHUNK];
                    float w[UNROLL];
#pragma unroll
                    for (int u = 0; u < UNROLL; ++u) {
                        const int tt = t + u;
                        const int32_t c = __shfl(c0[ki], tt & (LPR - 1), LPR);
                        const auto* xr = x_row(a, c) + col00;
#pragma unroll
                        for (int k = 0; k < NCHUNK; ++k) {
                            const int col = (k * LPR + gl) * VEC;
                            if (tt < nk && col < a.d) v[u][k].load(xr + col);
                            else v[u][k].zero();
                        }
                    }
#pragma unroll
                    for (int u = 0; u < UNROLL; ++u) {
                        if (WEIGHTED) w[u] = __shfl(w0[ki], (t + u) & (LPR - 1), LPR);
#pragma unroll
                        for (int k = 0; k < NCHUNK; ++k) {
                            if (WEIGHTED) acc[k].fma(w[u], v[u][k]);
                            else acc[k].add(v[u][k]);
                        }
                    }
                }
            }
            finish_row<LPR, NCHUNK, VEC>(a, col00, row0, gl, acc, false);
        }
        if (!has1) break;
        row0 = row1; col00 = col01; s0 = s1; n0 = n1;
#pragma unroll
        for (int k = 0; k < NI; ++k) c0[k] = c1[k];
        row1 = row2; col01 = col02; s1 = s2; n1 = n2;
        t1 = t2; has1 = has2;
    }
}

// The pipelined short rows of the SLICE-MASKED product (SpmmArgs.smask: the step's in-place side product, whose attribute slices of X are
// zero outside the rows the loss launch stamped). The mask bytes depend on the column indices, so the pipeline is one stage deeper than
// rows_body_pipe: the row pointers of task i + 3, the indices of task i + 2 and the mask bytes of task i + 1 are in flight while the rows
// of task i are gathered - still one round trip per task. An inactive column becomes index -1 and its gather is predicated off: the
// value that enters the fma chain is the +0 the promised-zero row would have delivered, so the sums are the unmasked product's, bit for
// bit. A masked task whose lane group sees no active column gathers nothing; in the in-place form it leaves its row untouched
// (Y[r] + 0 = Y[r]). Tasks below smask_col0 run as in rows_body_pipe. Any task count per lane group (pipe >= 1). The weights are
// col_scale (the host admits pattern-only operands weighted by it): a stage carries two words, and the kernel keeps its host's 5 waves.
template <int LPR, int NCHUNK, int VEC>
__device__ __forceinline__ void rows_body_pipe_smask(const SpmmArgs& a, int64_t block, int64_t n_blocks) {
    constexpr int GPB = TPB / LPR;
    constexpr int NI = (LLMREC_SPMM_LONG_ROW + LPR - 1) / LPR;
    constexpr int NBITS = 6, NMAX = LLMREC_SPMM_LONG_ROW + 1;           // a task's (slice, min(nnz, NMAX)) in one register: slice << NBITS | nnz
    static_assert(NMAX < (1 << NBITS), "rows_body_pipe_smask: the row length does not fit its bits");
    const int gl = threadIdx.x & (LPR - 1);
    const int g0 = (int)(threadIdx.x & 63) / LPR * LPR;
    const int32_t n_list = (int32_t)(a.slot_row ? (int64_t)a.n_short_rows : a.n_rows);      // (32-bit task ids: checked by the host)
    const int32_t n_tasks = n_list * a.n_slices, G = (int32_t)n_blocks * GPB;
    const int32_t t0 = (int32_t)block * GPB + (int32_t)(threadIdx.x / LPR);
    if (t0 >= n_tasks) return;
    const int32_t stamp = a.smask ? (int32_t)LLMREC_ROW_STAMP(a.smask_stamp[0]) : 0;        // (uniform)
    auto level1 = [&](int32_t t, int32_t& s_, int32_t& sn) {                                  // the row pointers
        const int32_t slice = t / n_list, slot = t - slice * n_list;
        s_ = a.rowptr[slot];
        sn = slice << NBITS | min(a.rowptr[slot + 1] - s_, NMAX);
    };
    auto level2 = [&](int32_t s_, int32_t sn, int32_t (&c)[NI]) {                             // the row's column indices (<= LONG_ROW of them)
        const int32_t n_ = sn & 63;
#pragma unroll
        for (int k = 0; k < NI; ++k) { const int j = k * LPR + gl; c[k] = (j < n_ && n_ <= LLMREC_SPMM_LONG_ROW) ? a.colidx[s_ + j] : 0; }
    };
    auto level3 = [&](int32_t sn, const int32_t (&c)[NI], int32_t (&m)[NI]) {                 // the columns' mask bytes (masked slices only)
        const int32_t n_ = sn & 63;
#pragma unroll
        for (int k = 0; k < NI; ++k) {
            const int j = k * LPR + gl;
            m[k] = stamp;
            if ((sn >> NBITS) * a.d >= a.smask_col0 && j < n_ && n_ <= LLMREC_SPMM_LONG_ROW) m[k] = (int32_t)a.smask[c[k]];
        }
    };
    int32_t snD, cD[NI];                                                // task i: gathers (inactive columns: -1)
    int32_t sC = 0, snC = 0, cC[NI], mC[NI];                            // task i + 1: mask bytes
    int32_t sB = 0, snB = 0;                                            // task i + 2: indices
#pragma unroll
    for (int k = 0; k < NI; ++k) { cC[k] = 0; mC[k] = 0; }
    int32_t t2 = t0 + 2 * G;
    bool has1 = t0 + G < n_tasks, has2 = has1 && t2 < n_tasks;
    int32_t sD;
    level1(t0, sD, snD);                                                // prologue: the first task's three dependent levels, the second's two,
    if (has1) level1(t0 + G, sC, snC);                                  // the third's one
    if (has2) level1(t2, sB, snB);
    level2(sD, snD, cD);
    if (has1) level2(sC, snC, cC);
    level3(snD, cD, mC);
#pragma unroll
    for (int k = 0; k < NI; ++k) cD[k] = mC[k] == stamp ? cD[k] : -1;
    for (;;) {
        int32_t sA = 0, snA = 0, cB[NI];
        const int32_t t3 = t2 + G;
        const bool has3 = has2 && t3 < n_tasks;
#pragma unroll
        for (int k = 0; k < NI; ++k) cB[k] = 0;
        if (has2) level2(sB, snB, cB);                                  // in flight while task i's rows are gathered
        if (has3) level1(t3, sA, snA);
        if (has1) level3(snC, cC, mC);
        const int32_t nD = snD & 63, sliceD = snD >> NBITS, colD = sliceD * a.d;
        if (nD <= LLMREC_SPMM_LONG_ROW) {                               // (longer: a row of another bucket, plain plans only)
            bool any = true;
            if (colD >= a.smask_col0) {                                 // (uniform per lane group) a masked task: does the row have an active column?
                bool act = false;
#pragma unroll
                for (int k = 0; k < NI; ++k) act |= k * LPR + gl < nD && cD[k] >= 0;
                any = ((__ballot(act) >> g0) & ((1ull << LPR) - 1ull)) != 0ull;
            }
            if (any || !a.smask_inplace) {
                const int32_t slotD = (t2 - 2 * G) - sliceD * n_list;
                const int32_t rowD = a.slot_row ? a.slot_row[slotD] : slotD;       // (the output row: beside the gathers, read behind them)
                float w0[NI];
#pragma unroll
                for (int k = 0; k < NI; ++k) w0[k] = (k * LPR + gl < nD && cD[k] >= 0) ? a.col_scale[cD[k]] : 0.f;
                Vec<VEC> acc[NCHUNK];
#pragma unroll
                for (int k = 0; k < NCHUNK; ++k) acc[k].zero();
#pragma unroll
                for (int ki = 0; ki < NI; ++ki) {
                    const int nk = any ? min(LPR, nD - ki * LPR) : 0;   // (uniform per lane group)
                    for (int t = 0; t < nk; t += UNROLL) {
                        Vec<VEC> v[UNROLL][NCHUNK];
                        float w[UNROLL];
#pragma unroll
                        for (int u = 0; u < UNROLL; ++u) {
                            const int tt = t + u;
                            const int32_t c = __shfl(cD[ki], tt & (LPR - 1), LPR);
                            const float* xr = a.X + (int64_t)c * a.ldx + colD;
#pragma unroll
                            for (int k = 0; k < NCHUNK; ++k) {
                                const int col = (k * LPR + gl) * VEC;
                                if (tt < nk && c >= 0 && col < a.d) v[u][k].load(xr + col);
                                else v[u][k].zero();
                            }
                        }
#pragma unroll
                        for (int u = 0; u < UNROLL; ++u) {
                            w[u] = __shfl(w0[ki], (t + u) & (LPR - 1), LPR);
#pragma unroll
                            for (int k = 0; k < NCHUNK; ++k) acc[k].fma(w[u], v[u][k]);
                        }
                    }
                }
                finish_row<LPR, NCHUNK, VEC>(a, colD, rowD, gl, acc, false);
            }
        }
        if (!has1) break;
        snD = snC;
#pragma unroll
        for (int k = 0; k < NI; ++k) { cD[k] = mC[k] == stamp ? cC[k] : -1; cC[k] = cB[k]; }
        sC = sB; snC = snB;
        sB = sA; snB = snA;
        t2 = t3; has1 = has2; has2 = has3;
    }
}

// one wavefront over [s, e): the 64/LPR lane groups take contiguous parts, butterfly sum -> every group holds the total
template <int LPR, int NCHUNK, int VEC, bool WEIGHTED, bool MASKED, class A>
__device__ __forceinline__ void wave_range(const A& a, int64_t col0, int32_t s, int32_t e, int lane, Vec<VEC> (&acc)[NCHUNK], int& any,
                                           const uint8_t* xm, int xa) {
    constexpr int G = 64 / LPR;
    const int gl = lane & (LPR - 1), g = lane / LPR;
    const int32_t per = (((e - s) + G - 1) / G + LPR - 1) / LPR * LPR;      // multiple of LPR: aligned index loads
    const int32_t gs = min(s + g * per, e), ge = min(gs + per, e);
#pragma unroll
    for (int k = 0; k < NCHUNK; ++k) acc[k].zero();
    accumulate_range<LPR, NCHUNK, VEC, WEIGHTED, MASKED>(a, col0, gs, ge, gl, acc, any, xm, xa);
#pragma unroll
    for (int off = LPR; off < 64; off <<= 1) {
#pragma unroll
        for (int k = 0; k < NCHUNK; ++k) acc[k].xor_add(off);
    }
}

// (row, slice) tasks of a row list, slice-major
// crow: the row of the CSR arrays (a slot of the permuted CSR when there is one), row: the output row
__device__ __forceinline__ void list_task(const SpmmArgs& a, const int32_t* list, int32_t n_list, int64_t task, int32_t& crow, int32_t& row, int64_t& col0, int32_t& slot) {
    const int64_t slice = task / n_list;
    slot = (int32_t)(task - slice * n_list);
    crow = list[slot];
    row = a.slot_row ? a.slot_row[crow] : crow;
    col0 = slice * a.d;
}

// one wavefront per (row, slice) of the wave-row list
template <int LPR, int NCHUNK, int VEC, bool WEIGHTED, bool MASKED, int BT = TPB, class A>
__device__ __forceinline__ void wave_rows_body(const A& a, int32_t block) {
    const int lane = threadIdx.x & 63;
    const int64_t task = (int64_t)block * (BT / 64) + (threadIdx.x >> 6);
    if (task >= (int64_t)a.n_wave_rows * a.n_slices) return;
    int32_t crow, row, slot; int64_t col0;
    list_task(a, a.wave_rows, a.n_wave_rows, task, crow, row, col0, slot);
    Vec<VEC> acc[NCHUNK];
    int any = 0;
    bool zero_row = false;
    if (MASKED) {                                                        // as in rows_body: scan the mask first, accumulate only if something is active
        const int32_t rs = a.rowptr[crow], re = a.rowptr[crow + 1];
        for (int32_t base = rs; base < re; base += 64)
            if (base + lane < re) any |= (int)a.x_mask[a.colidx[base + lane]] == a.x_active;
        const bool any_w = __ballot(any != 0) != 0ull;
        zero_row = write_row_flag(a, row, any_w, col0 == 0 && lane == 0);
        if (any_w) wave_range<LPR, NCHUNK, VEC, WEIGHTED, MASKED>(a, col0, rs, re, lane, acc, any, a.x_mask, a.x_active);
        else {
#pragma unroll
            for (int k = 0; k < NCHUNK; ++k) acc[k].zero();
        }
    } else {
        wave_range<LPR, NCHUNK, VEC, WEIGHTED, MASKED>(a, col0, a.rowptr[crow], a.rowptr[crow + 1], lane, acc, any, a.x_mask, a.x_active);
    }
    if (lane < LPR) finish_row<LPR, NCHUNK, VEC>(a, col0, row, lane, acc, zero_row);
}

// wave_rows_body of the slice-masked product (SpmmArgs.smask): a task at or beyond smask_col0 scans its columns' mask bytes first and gathers
// the active ones only (the masked loop: ascending, the skipped terms are exact +0); without an active column the in-place form leaves
// the row untouched. Tasks of lower slices run the plain loop.
template <int LPR, int NCHUNK, int VEC, bool WEIGHTED>
__device__ __forceinline__ void wave_rows_body_smask(const SpmmArgs& a, int32_t block) {
    const int lane = threadIdx.x & 63;
    const int64_t task = (int64_t)block * (TPB / 64) + (threadIdx.x >> 6);
    if (task >= (int64_t)a.n_wave_rows * a.n_slices) return;
    int32_t crow, row, slot; int64_t col0;
    list_task(a, a.wave_rows, a.n_wave_rows, task, crow, row, col0, slot);
    const int32_t rs = a.rowptr[crow], re = a.rowptr[crow + 1];
    Vec<VEC> acc[NCHUNK];
    int any = 0;
    if (col0 >= a.smask_col0) {                                          // (wave-uniform)
        const int stamp = (int)LLMREC_ROW_STAMP(a.smask_stamp[0]);
        for (int32_t base = rs; base < re; base += 64)
            if (base + lane < re) any |= (int)a.smask[a.colidx[base + lane]] == stamp;
        if (__ballot(any != 0) != 0ull) wave_range<LPR, NCHUNK, VEC, WEIGHTED, true>(a, col0, rs, re, lane, acc, any, a.smask, stamp);
        else if (a.smask_inplace) return;
        else {
#pragma unroll
            for (int k = 0; k < NCHUNK; ++k) acc[k].zero();
        }
    } else {
        wave_range<LPR, NCHUNK, VEC, WEIGHTED, false>(a, col0, rs, re, lane, acc, any, nullptr, 0);
    }
    if (lane < LPR) finish_row<LPR, NCHUNK, VEC>(a, col0, row, lane, acc, false);
}

// one block over [s, e): the 8 waves take contiguous parts, summed through LDS in wave order; the total ends up in the
// first lane group of wave 0 (returns true there)
template <int LPR, int NCHUNK, int VEC, bool WEIGHTED, bool MASKED, class A>
__device__ __forceinline__ bool block_range(const A& a, int64_t col0, int32_t s, int32_t e, float* lds, Vec<VEC> (&acc)[NCHUNK],
                                            const uint8_t* xm, int xa) {
    constexpr int ROWW = NCHUNK * LPR * VEC;
    constexpr int NW = TPB / 64;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int32_t per = (((e - s) + NW - 1) / NW + 63) / 64 * 64;
    const int32_t ws = min(s + w * per, e), we = min(ws + per, e);
    int any = 0;                                                         // (long rows: their output flag is set unconditionally)
    wave_range<LPR, NCHUNK, VEC, WEIGHTED, MASKED>(a, col0, ws, we, lane, acc, any, xm, xa);
    if (w > 0 && lane < LPR) {
#pragma unroll
        for (int k = 0; k < NCHUNK; ++k) acc[k].store(lds + (w - 1) * ROWW + (k * LPR + lane) * VEC);
    }
    __syncthreads();
    if (w != 0 || lane >= LPR) return false;
#pragma unroll
    for (int ww = 0; ww < NW - 1; ++ww) {
#pragma unroll
        for (int k = 0; k < NCHUNK; ++k) { Vec<VEC> o; o.load(lds + ww * ROWW + (k * LPR + lane) * VEC); acc[k].add(o); }
    }
    return true;
}

// block_range (unmasked) in a block of BT < TPB threads: the row is still cut into TPB / 64 parts and each of the block's BT / 64
// wavefronts runs its share of them in turn - part p by wavefront p % (BT / 64), into the LDS slot part p has in the 512-thread block
// (part 0 stays in registers) - followed by the same additions in the same order: the summation tree of block_range, bit for bit.
template <int LPR, int NCHUNK, int VEC, bool WEIGHTED, int BT>
__device__ __forceinline__ bool block_range_bt(const SpmmArgs& a, int64_t col0, int32_t s, int32_t e, float* lds, Vec<VEC> (&acc)[NCHUNK]) {
    constexpr int ROWW = NCHUNK * LPR * VEC;
    constexpr int NW = TPB / 64, PW = BT / 64;
    static_assert(BT % 64 == 0 && NW % PW == 0, "block_range_bt: the block's wavefronts share the 8 parts evenly");
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int32_t per = (((e - s) + NW - 1) / NW + 63) / 64 * 64;
    Vec<VEC> first[NCHUNK];                                              // part 0 (wavefront 0, first turn)
    int any = 0;
#pragma unroll
    for (int turn = 0; turn < NW / PW; ++turn) {
        const int p = w + turn * PW;
        const int32_t ws = min(s + p * per, e), we = min(ws + per, e);
        wave_range<LPR, NCHUNK, VEC, WEIGHTED, false>(a, col0, ws, we, lane, acc, any, nullptr, 0);
        if (p > 0 && lane < LPR) {
#pragma unroll
            for (int k = 0; k < NCHUNK; ++k) acc[k].store(lds + (p - 1) * ROWW + (k * LPR + lane) * VEC);
        }
        if (turn == 0) {
#pragma unroll
            for (int k = 0; k < NCHUNK; ++k) first[k] = acc[k];
        }
    }
    __syncthreads();
    if (w != 0 || lane >= LPR) return false;
#pragma unroll
    for (int k = 0; k < NCHUNK; ++k) acc[k] = first[k];
#pragma unroll
    for (int ww = 0; ww < NW - 1; ++ww) {
#pragma unroll
        for (int k = 0; k < NCHUNK; ++k) { Vec<VEC> o; o.load(lds + ww * ROWW + (k * LPR + lane) * VEC); acc[k].add(o); }
    }
    return true;
}

// block_range of the slice-masked product: the masked loop at or beyond smask_col0 (block-uniform), the plain one below
template <int LPR, int NCHUNK, int VEC, bool WEIGHTED>
__device__ __forceinline__ bool block_range_smask(const SpmmArgs& a, int64_t col0, int32_t s, int32_t e, float* lds, Vec<VEC> (&acc)[NCHUNK]) {
    if (col0 >= a.smask_col0)
        return block_range<LPR, NCHUNK, VEC, WEIGHTED, true>(a, col0, s, e, lds, acc, a.smask, (int)LLMREC_ROW_STAMP(a.smask_stamp[0]));
    return block_range<LPR, NCHUNK, VEC, WEIGHTED, false>(a, col0, s, e, lds, acc, nullptr, 0);
}

// One problem's block b (a global block id) of the ranges of SpmmArgs: the heavy blocks come first. The segment partials are indexed by
// the problem-local block id, so a grouped launch addresses them exactly like a launch of its own.
// SMASK (with MASKED = false): the slice-masked product - the run-time choice between the plain and the masked loops per task.
template <int LPR, int NCHUNK, int VEC, bool WEIGHTED, bool MASKED, bool SMASK = false, class A>
__device__ __forceinline__ void spmm_body(const A& a, int32_t b, float* red_lds) {
    static_assert(!SMASK || (WEIGHTED && !MASKED), "spmm_body: the slice-masked product is weighted and has no host-stamped mask");
    if (b >= a.blk_wave) {
        const int64_t lb = (int64_t)b - a.blk_wave;
        if constexpr (SMASK) rows_body_pipe_smask<LPR, NCHUNK, VEC>(a, lb, (int64_t)a.blk_end - a.blk_wave);
        else if (!MASKED && a.pipe > 1) rows_body_pipe<LPR, NCHUNK, VEC, WEIGHTED>(a, lb, (int64_t)a.blk_end - a.blk_wave);     // (block-uniform)
        else rows_body<LPR, NCHUNK, VEC, WEIGHTED, MASKED>(a, lb);
        return;
    }
    if (b >= a.blk_block) {
        if constexpr (SMASK) wave_rows_body_smask<LPR, NCHUNK, VEC, WEIGHTED>(a, b - a.blk_block);
        else wave_rows_body<LPR, NCHUNK, VEC, WEIGHTED, MASKED>(a, b - a.blk_block);
        return;
    }
    Vec<VEC> acc[NCHUNK];
    int32_t crow, row, slot; int64_t col0;
    if (b >= a.blk_seg) {
        list_task(a, a.block_rows, a.n_block_rows, b - a.blk_seg, crow, row, col0, slot);
        bool mine;                                                       // (long rows of the slice-masked product are always computed and written)
        if constexpr (SMASK) mine = block_range_smask<LPR, NCHUNK, VEC, WEIGHTED>(a, col0, a.rowptr[crow], a.rowptr[crow + 1], red_lds, acc);
        else mine = block_range<LPR, NCHUNK, VEC, WEIGHTED, MASKED>(a, col0, a.rowptr[crow], a.rowptr[crow + 1], red_lds, acc, a.x_mask, a.x_active);
        if (mine) {
            if (MASKED && col0 == 0 && threadIdx.x == 0 && a.y_flag) a.y_flag[row] = (uint8_t)a.x_active;   // conservative: "may be non-zero"
            finish_row<LPR, NCHUNK, VEC>(a, col0, row, threadIdx.x, acc);
        }
        return;
    }
    const int32_t lb = b - a.blk_begin;
    const int32_t slice = lb / a.n_segments, seg = lb - slice * a.n_segments;
    slot = a.seg_split[seg];
    crow = a.split_rows[slot];
    row = a.slot_row ? a.slot_row[crow] : crow;
    col0 = (int64_t)slice * a.d;
    const int32_t k_in_row = seg - a.split_seg_begin[slot];
    const int32_t re = a.rowptr[crow + 1];
    const int32_t s = a.rowptr[crow] + k_in_row * a.segment;
    const int32_t e = min(s + a.segment, re);
    bool mine;
    if constexpr (SMASK) mine = block_range_smask<LPR, NCHUNK, VEC, WEIGHTED>(a, col0, s, e, red_lds, acc);
    else mine = block_range<LPR, NCHUNK, VEC, WEIGHTED, MASKED>(a, col0, s, e, red_lds, acc, a.x_mask, a.x_active);
    if (mine) {
        if (MASKED && col0 == 0 && k_in_row == 0 && threadIdx.x == 0 && a.y_flag) a.y_flag[row] = (uint8_t)a.x_active;   // conservative
        float* pr = a.partials + (int64_t)lb * a.d;
#pragma unroll
        for (int k = 0; k < NCHUNK; ++k) {
            const int col = (k * LPR + (int)threadIdx.x) * VEC;
            if (col < a.d) acc[k].store(pr + col);
        }
    }
}

// The finalize launch of the split rows. One block of 256 threads per (split row, slice): the 256/LPR lane groups each add every
// (256/LPR)-th segment partial (ascending), then the groups are combined through LDS in group order - a fixed summation tree; then the
// row's epilogue
template <int LPR, int NCHUNK, int VEC, class A>
__device__ __forceinline__ void spmm_finalize_body(const A& a, int32_t blk, float* fin_lds) {
    constexpr int G = 256 / LPR;
    constexpr int ROWW = NCHUNK * LPR * VEC;
    const int gl = threadIdx.x & (LPR - 1), g = threadIdx.x / LPR;
    const int32_t slice = blk / a.n_split_rows, slot = blk - slice * a.n_split_rows;
    const int32_t crow = a.split_rows[slot];
    const int32_t row = a.slot_row ? a.slot_row[crow] : crow;
    const int32_t deg = a.rowptr[crow + 1] - a.rowptr[crow];
    const int32_t nseg = (deg + a.segment - 1) / a.segment;
    const float* pr = a.partials + ((int64_t)slice * a.n_segments + a.split_seg_begin[slot]) * a.d;
    Vec<VEC> acc[NCHUNK];
#pragma unroll
    for (int k = 0; k < NCHUNK; ++k) acc[k].zero();
    for (int s0 = g; s0 < nseg; s0 += G) {
#pragma unroll
        for (int k = 0; k < NCHUNK; ++k) {
            const int col = (k * LPR + gl) * VEC;
            if (col < a.d) { Vec<VEC> v; v.load(pr + (int64_t)s0 * a.d + col); acc[k].add(v); }
        }
    }
#pragma unroll
    for (int k = 0; k < NCHUNK; ++k) acc[k].store(fin_lds + g * ROWW + (k * LPR + gl) * VEC);
    __syncthreads();
    if (g != 0) return;
#pragma unroll
    for (int k = 0; k < NCHUNK; ++k) {
        acc[k].zero();
        for (int gg = 0; gg < G; ++gg) { Vec<VEC> o; o.load(fin_lds + gg * ROWW + (k * LPR + gl) * VEC); acc[k].add(o); }
    }
    finish_row<LPR, NCHUNK, VEC>(a, (int64_t)slice * a.d, row, gl, acc);
}

// spmm_body for a product HOSTED by another kernel's launch of BT-thread blocks: unmasked, no split rows (the host of the launch refuses
// such a plan: blk_seg == blk_begin), block b of a layout made for BT threads (spmm_layout). red_lds: (TPB / 64 - 1) rows of floats.
template <int LPR, int NCHUNK, int VEC, bool WEIGHTED, int BT>
__device__ __forceinline__ void spmm_hosted_body(const SpmmArgs& a, int32_t b, float* red_lds) {
    if (b >= a.blk_wave) {
        const int64_t lb = (int64_t)b - a.blk_wave;
        if (a.pipe > 1) rows_body_pipe<LPR, NCHUNK, VEC, WEIGHTED, BT>(a, lb, (int64_t)a.blk_end - a.blk_wave);     // (block-uniform)
        else rows_body<LPR, NCHUNK, VEC, WEIGHTED, false, BT>(a, lb);
        return;
    }
    if (b >= a.blk_block) {
        wave_rows_body<LPR, NCHUNK, VEC, WEIGHTED, false, BT>(a, b - a.blk_block);
        return;
    }
    Vec<VEC> acc[NCHUNK];
    int32_t crow, row, slot; int64_t col0;
    list_task(a, a.block_rows, a.n_block_rows, b - a.blk_seg, crow, row, col0, slot);
    if (block_range_bt<LPR, NCHUNK, VEC, WEIGHTED, BT>(a, col0, a.rowptr[crow], a.rowptr[crow + 1], red_lds, acc))
        finish_row<LPR, NCHUNK, VEC>(a, col0, row, threadIdx.x, acc);
}

// host side of a hosted product (spmm.hip: spmm_prepare_hosted): the arguments laid out from block 0 for blocks of the host's size,
// the block count, and the extents of what the product reads (X, Z) and writes (Y) for the host's aliasing check.
// weighted: which of the two hosted shapes it is - false: the plain product (spmm_hosted_body<.., false, ..>: the projection's guest);
// true: the product weighted by col_scale alone, with or without the init term alpha Z (<.., true, ..>: the weight gradient's guest).
struct SpmmHosted {
    SpmmArgs a;
    int64_t blocks, bytes_x, bytes_y, bytes_z;
    bool weighted;
};
int spmm_prepare_hosted(const llmrec_spmm_problem_t& pr, int tpb, SpmmHosted& out);

// host side of a single product launched by another translation unit (spmm_bf16.hip, whose X is not an fp32 tensor: pr.X = NULL, pr.ldx =
// the operand's ld): the checks of llmrec_spmm_f32, the kernel family (spmm.hip: 0..4 = the float4 families of up to 16 / 32 / 64 / 128 /
// 256 columns), whether the operand is weighted, and the arguments laid out as a launch of their own with its block count
struct SpmmSingle {
    SpmmArgs a;
    int family;
    bool weighted, empty;
    int64_t blocks;
};
int spmm_prepare_single(const llmrec_spmm_problem_t& pr, SpmmSingle& out);

}  // namespace llmrec
