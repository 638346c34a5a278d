// mask.hip - the fused step's feature masking and attribute restoration (reference Models.py:130-142, main.py:258-273), opt-in:
//   llmrec_mask_nodes        the round's list of distinct masked rows: the sampler's keyed bijection (guests.h) under a key of its own
//   llmrec_col_sums_f64      fp64 column sums of up to 8 equally shaped tensors, from scratch (set-up / refresh)
//   llmrec_mask_rows_f32     one masking round: the listed rows become the column mean, the running sums follow without a re-read
//   llmrec_restore_loss_f32  the restoration loss of up to 8 streams that share a node list and a decoder, and its gradient rows
//   llmrec_restore_finish_f32  the logged scalars' share of the term and the row-wise clean-up of the gradient's scatter rows
// Every contract is stated in full on the declaration (include/llmrec_hip.h, R13). No float atomics, 64-bit element offsets, no scratch.
//
// Column sums and masking share one geometry: a block is 32 consecutive columns x LLMREC_MASK_ROW_LANES = 8 row lanes (a row lane's 32
// threads read one 128-byte segment of a row), row lane j walks rows / list entries j, j + 8, ... in ascending order in fp64 and the
// eight partial sums are added in ascending j. A column belongs to ONE block, so a round needs no hand-over between blocks, and the
// tree does not depend on the grid. The fp64 update is written without contraction: the header states every rounding.
//
// The restoration kernel: one wavefront owns 16 list rows and walks F in tiles of 16 with v_mfma_f32_16x16x4_f32 (exact fp32, a k-ordered
// fma chain - dense.hip). The first product is taken TRANSPOSED, Y^T = W_tile X^T, so that its accumulator - lane (r, q) holds
// y[f = 4 q + i][row r] in register i - is, unchanged, the B operand of the products that sum over f: p^T += W_tile^T Y^T and, with the
// target tile loaded in the same layout (one float4 per lane), q^T += W_tile^T T^T. Nothing of size [rows, F] leaves the registers.
#include "common.h"
#include "guests.h"
#include <math.h>

namespace llmrec {

constexpr uint64_t MASK_KEY = 0x6A09E667F3BCC908ull;                  // seed ^ this: beside the sampler's two keys and the dropout key
constexpr int MASK_LANES = LLMREC_MASK_ROW_LANES, MASK_COLS = 32;
static_assert(MASK_LANES * MASK_COLS == 256, "a block of mask_rows / col_sums is 32 columns x 8 row lanes");

__global__ __launch_bounds__(256) void mask_nodes_kernel(int64_t N, int64_t m, int half_bits, uint64_t key, unsigned long long* step_dev,
                                                         uint32_t side, int64_t* __restrict__ nodes, int32_t* ticket) {
    const unsigned long long step = *step_dev;
    const unsigned long long word = 2ull * step + side;                 // (mod 2^64)
    const Philox ph(key);
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j < m) nodes[j] = (int64_t)keyed_perm((uint64_t)j, (uint64_t)N, half_bits, ph, (uint32_t)word, (uint32_t)(word >> 32));
    if (ticket == nullptr) return;                                      // (uniform) the launch only reads the counter
    __syncthreads();                                                    // every thread of this block is done with the round's value
    if (threadIdx.x == 0) {
        __threadfence();
        if (atomicAdd(ticket, 1) == (int)gridDim.x - 1) {               // the last block: every block has read the counter
            *step_dev = step + 1ull;
            atomicExch(ticket, 0);
        }
    }
}

struct MaskTensors {
    float* X[LLMREC_MASK_MAX_TENSORS];
    double* sums[LLMREC_MASK_MAX_TENSORS];
};

__global__ __launch_bounds__(256) void col_sums_kernel(MaskTensors a, int64_t N, int cols, int64_t ldx) {
    __shared__ double part[MASK_LANES][MASK_COLS];
    const int tx = threadIdx.x & (MASK_COLS - 1), j = threadIdx.x / MASK_COLS;
    const int c = blockIdx.x * MASK_COLS + tx;
    const float* __restrict__ X = a.X[blockIdx.y];
    double acc = 0.0;
    if (c < cols)
        for (int64_t r = j; r < N; r += MASK_LANES) acc = acc + (double)X[r * ldx + c];
    part[j][tx] = acc;
    __syncthreads();
    if (j == 0 && c < cols) {
        double s = part[0][tx];
#pragma unroll
        for (int k = 1; k < MASK_LANES; ++k) s = s + part[k][tx];
        a.sums[blockIdx.y][c] = s;
    }
}

__global__ __launch_bounds__(256) void mask_rows_kernel(MaskTensors a, int64_t N, int cols, int64_t ldx, const int64_t* __restrict__ nodes,
                                                        int64_t m) {
#pragma clang fp contract(off)
    __shared__ double part[MASK_LANES][MASK_COLS];
    const int tx = threadIdx.x & (MASK_COLS - 1), j = threadIdx.x / MASK_COLS;
    const int c = blockIdx.x * MASK_COLS + tx;
    float* X = a.X[blockIdx.y];
    double* sums = a.sums[blockIdx.y];
    const bool ok = c < cols;                                           // columns [cols, ldx) are never touched
    const double sum = ok ? sums[c] : 0.0;
    const float mean = (float)(sum / (double)N);
    double acc = 0.0;
    if (ok) {                                                           // each (row, column) element belongs to one thread: the list is duplicate-free
        int64_t i = j;
        for (; i + 3 * MASK_LANES < m; i += 4 * MASK_LANES) {           // four entries' loads in flight; the additions keep the list order
            float* p[4];
            float v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) p[k] = X + nodes[i + k * MASK_LANES] * ldx + c;
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = *p[k];
#pragma unroll
            for (int k = 0; k < 4; ++k) { acc = acc + (double)v[k]; *p[k] = mean; }
        }
        for (; i < m; i += MASK_LANES) {
            float* p = X + nodes[i] * ldx + c;
            acc = acc + (double)*p;
            *p = mean;
        }
    }
    part[j][tx] = acc;
    __syncthreads();
    if (j == 0 && ok) {
        double old = part[0][tx];
#pragma unroll
        for (int k = 1; k < MASK_LANES; ++k) old = old + part[k][tx];
        const double put = (double)m * (double)mean;
        const double delta = put - old;
        sums[c] = sum + delta;
    }
}

// ---------------------------------------------------------------------------------------------
// restoration
// ---------------------------------------------------------------------------------------------
struct RestoreArgs {
    const float* X[LLMREC_MASK_MAX_TENSORS];
    const float* T[LLMREC_MASK_MAX_TENSORS];
    float* dX[LLMREC_MASK_MAX_TENSORS];
    int64_t ldx, ldt, lddx, ldw, m;
    const int64_t* nodes;
    const float* W;
    const float* b;
    int F, loss_type, vec_x, vec_t, vec_w, vec_dx;
    float alpha, scale;
    float* row_loss;
    uint8_t* row_flags;
    const int32_t* row_stamp;
};

__device__ __forceinline__ float pow_int_or(float base, float alpha) {  // alpha 1, 2, 3: products; else powf
    if (alpha == 1.f) return base;
    if (alpha == 2.f) return base * base;
    if (alpha == 3.f) return base * base * base;
    return powf(base, alpha);
}

template <bool GRAD>
__global__ __launch_bounds__(256) void restore_rows_kernel(RestoreArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 15, lq = lane >> 4;
    const int64_t r0 = ((int64_t)blockIdx.x * 4 + wave) * 16;
    if (r0 >= a.m) return;                                              // (wavefront-uniform; the kernel has no block barrier)
    const int s = blockIdx.y, F = a.F;
    const int64_t r = r0 + li;
    const bool live = r < a.m;
    const int64_t node = a.nodes[live ? r : a.m - 1];                   // a dead lane repeats the last row and writes nothing
    const float* __restrict__ xrow = a.X[s] + node * a.ldx;
    const float* __restrict__ trow = a.T[s] + node * a.ldt;
    const float* __restrict__ W = a.W;
    float4 xb[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) xb[j] = load4_guard(xrow, 16 * j + 4 * lq, 64, a.vec_x);
    f32x4 pacc[4], qacc[4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) { pacc[kt] = (f32x4){0.f, 0.f, 0.f, 0.f}; qacc[kt] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
    float syy = 0.f, syt = 0.f, stt = 0.f;
    // a tile's operands: W's rows f0 + li (the first product's A operand), the target's columns f0 + 4 lq .. + 3 and, with the
    // gradient, W[f0 + 4 lq + i][16 kt + li] (the A operand of the products that sum over f). They are loaded ONE TILE AHEAD, so that
    // the loads of tile n + 1 are in flight under the MFMAs of tile n; behind the last tile it is loaded once more, unused.
    float4 wa[4], wa_n[4], tb, tb_n;
    float wt[4][4], wt_n[4][4];
    auto load_tile = [&](int f0, float4 (&wa_)[4], float4& tb_, float (&wt_)[4][4]) {
        const int fa = f0 + li < F ? f0 + li : F - 1;
        const float* __restrict__ wrow = W + (int64_t)fa * a.ldw;
#pragma unroll
        for (int j = 0; j < 4; ++j) wa_[j] = load4_guard(wrow, 16 * j + 4 * lq, 64, a.vec_w);
        tb_ = load4_guard(trow, f0 + 4 * lq, F, a.vec_t);
        if (GRAD) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int f = f0 + 4 * lq + i;
                const float* __restrict__ wf = W + (int64_t)(f < F ? f : F - 1) * a.ldw;
#pragma unroll
                for (int kt = 0; kt < 4; ++kt) wt_[i][kt] = wf[16 * kt + li];
            }
        }
    };
    load_tile(0, wa, tb, wt);
    for (int f0 = 0; f0 < F; f0 += 16) {
        // Y^T tile: lane (li, lq) ends with y[f0 + 4 lq + i][row li] in acc[i]; the chain visits k = 16 j + 4 q + s in the order j, s, q
        load_tile(f0 + 16 < F ? f0 + 16 : f0, wa_n, tb_n, wt_n);
        f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(comp(wa[j], q), comp(xb[j], q), acc, 0, 0, 0);
        float y[4], t[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int f = f0 + 4 * lq + i;
            y[i] = f < F ? acc[i] + a.b[f] : 0.f;                       // past F: y = t = 0, so the tile's tail adds exact zeros
            t[i] = comp(tb, i);
            syy = fmaf(y[i], y[i], syy); syt = fmaf(y[i], t[i], syt); stt = fmaf(t[i], t[i], stt);
        }
        if (GRAD) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {                               // p^T += W_tile^T Y^T, q^T += W_tile^T T^T: f = f0 + 4 lq + i is the summed index
#pragma unroll
                for (int kt = 0; kt < 4; ++kt) {
                    pacc[kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wt[i][kt], y[i], pacc[kt], 0, 0, 0);
                    qacc[kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wt[i][kt], t[i], qacc[kt], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) wa[j] = wa_n[j];
        tb = tb_n;
        if (GRAD) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int kt = 0; kt < 4; ++kt) wt[i][kt] = wt_n[i][kt];
        }
    }
    // the three sums of row li: the lane's fma chain over its f's, then the four lq partials as (p ^ 16) and (p ^ 32) butterflies
    syy += __shfl_xor(syy, 16, 64); syy += __shfl_xor(syy, 32, 64);
    syt += __shfl_xor(syt, 16, 64); syt += __shfl_xor(syt, 32, 64);
    stt += __shfl_xor(stt, 16, 64); stt += __shfl_xor(stt, 32, 64);
    const float eps = 1e-12f;
    const float ry = sqrtf(syy), rt = sqrtf(stt);
    const float ny = fmaxf(ry, eps), nt = fmaxf(rt, eps);
    const float nn = ny * nt, cosv = syt / nn, ny2 = ny * ny;
    const float fm = (float)a.m;
    float loss, ca, cb;                                                 // dL/dy = ca t + cb y
    if (a.loss_type == LLMREC_RESTORE_SCE) {
        const float base = 1.f - cosv;
        loss = pow_int_or(base, a.alpha);
        const float g = a.alpha * (a.alpha == 1.f ? 1.f : pow_int_or(base, a.alpha - 1.f)) / fm;
        ca = -(g / nn);
        cb = ry >= eps ? g * cosv / ny2 : 0.f;
    } else {
        const float fF = (float)F;
        loss = ((syy / ny2 + stt / (nt * nt)) - 2.f * cosv) / fF;
        const float g = 2.f / (fm * fF);
        ca = -(g / nn);
        cb = (ry >= eps ? g * cosv : g) / ny2;
    }
    if (live && lq == 0) {
        a.row_loss[(int64_t)s * a.m + r] = loss;
        if (a.row_flags && s == 0) a.row_flags[node] = LLMREC_ROW_STAMP(a.row_stamp[0]);
    }
    if (GRAD && live) {
        float* __restrict__ drow = a.dX[s] + node * a.lddx;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {                                // lane (li, lq) holds columns 16 kt + 4 lq + i of row li
            const int k = 16 * kt + 4 * lq;
            float g[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) g[i] = a.scale * fmaf(cb, pacc[kt][i], ca * qacc[kt][i]);
            if (a.vec_dx) {
                float4 v = *reinterpret_cast<float4*>(drow + k);
                v.x += g[0]; v.y += g[1]; v.z += g[2]; v.w += g[3];
                *reinterpret_cast<float4*>(drow + k) = v;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) drow[k + i] += g[i];
            }
        }
    }
}

// one wavefront per stream: the 1024-slot tree of the loss launches (guests.h) over the stream's row losses, then / m
__global__ void restore_reduce_kernel(const float* __restrict__ row_loss, int64_t m, float* __restrict__ loss_out) {
    const int lane = threadIdx.x & 63, s = threadIdx.x >> 6;
    const float tot = wave_tree_sum_1024(row_loss + (int64_t)s * m, (int)m, lane);
    if (lane == 0) loss_out[s] = tot / (float)m;
}

struct FinishArgs {
    float* views[LLMREC_MASK_MAX_TENSORS];
    int n_views, cols;
    int64_t ld, m;
    const int64_t* nodes;
    const float* values;
    int n_values;
    float rate;
    float* scal;
    double* running;
};

// block 0: the logged scalars; blocks 1 ..: +0.0f into columns [0, cols) of the listed rows of every view, grid-stride over (view, row)
__global__ __launch_bounds__(256) void restore_finish_kernel(FinishArgs a) {
    if (blockIdx.x == 0) {
        if (threadIdx.x == 0 && a.n_values > 0) {
            float tot = a.values[0];
            for (int k = 1; k < a.n_values; ++k) tot += a.values[k];
            const float add = a.rate * tot;
            if (a.scal) a.scal[1] = a.scal[1] + add;
            if (a.running) a.running[0] = a.running[0] + (double)add;
        }
        return;
    }
    const int per_row = a.cols, rows_per_block = per_row >= 256 ? 1 : 256 / per_row;
    const int lr = per_row >= 256 ? 0 : (int)threadIdx.x / per_row, c0 = per_row >= 256 ? (int)threadIdx.x : (int)threadIdx.x % per_row;
    if (lr >= rows_per_block) return;
    const int64_t total = (int64_t)a.n_views * a.m;
    for (int64_t w = (int64_t)(blockIdx.x - 1) * rows_per_block + lr; w < total; w += (int64_t)(gridDim.x - 1) * rows_per_block) {
        float* row = a.views[w / a.m] + a.nodes[w % a.m] * a.ld;
        for (int c = c0; c < a.cols; c += 256) row[c] = 0.f;
    }
}

static int mask_tensors(int32_t n, float* const* X, double* const* sums, const char* who, MaskTensors& t) {
    LLMREC_CHECK_ARG(n >= 1 && n <= LLMREC_MASK_MAX_TENSORS && X && sums, "%s: 1 .. %d tensors with their sums expected", who,
                     LLMREC_MASK_MAX_TENSORS);
    t = MaskTensors{};
    for (int i = 0; i < n; ++i) {
        LLMREC_CHECK_ARG(X[i] && sums[i] && ((uintptr_t)X[i] & 3) == 0 && ((uintptr_t)sums[i] & 7) == 0, "%s: tensor %d: null or misaligned pointer", who, i);
        t.X[i] = X[i]; t.sums[i] = sums[i];
    }
    return LLMREC_OK;
}

}  // namespace llmrec

using namespace llmrec;

extern "C" {

int llmrec_mask_nodes(int64_t N, int64_t m, uint64_t seed, uint64_t* step_dev, int32_t side, int64_t* nodes, int32_t* ticket,
                      llmrec_stream_t stream_) {
    LLMREC_CHECK_ARG(N >= 1 && N < (1ll << 40) && m >= 0 && m <= N, "mask_nodes: N = %lld, m = %lld: 0 <= m <= N < 2^40 expected", (long long)N,
                     (long long)m);
    LLMREC_CHECK_ARG(side == LLMREC_MASK_SIDE_USERS || side == LLMREC_MASK_SIDE_ITEMS, "mask_nodes: side %d", (int)side);
    LLMREC_CHECK_ARG(step_dev && (m == 0 || nodes), "mask_nodes: null pointer");
    int hb = 1;
    while ((1ull << (2 * hb)) < (uint64_t)N) ++hb;
    const int64_t grid = m > 0 ? ceil_div(m, 256) : 1;
    mask_nodes_kernel<<<(unsigned)grid, 256, 0, (hipStream_t)stream_>>>(N, m, hb, seed ^ MASK_KEY, (unsigned long long*)step_dev, (uint32_t)side,
                                                                        nodes, ticket);
    LLMREC_LAUNCH_CHECK();
    return LLMREC_OK;
}

int llmrec_col_sums_f64(int32_t n_tensors, const float* const* X_host, int64_t ldx, double* const* sums_host, int64_t N, int32_t cols,
                        llmrec_stream_t stream_) {
    MaskTensors t;
    LLMREC_CHECK_ARG(N >= 1 && cols >= 1 && ldx >= cols, "col_sums: bad sizes");
    if (int st = mask_tensors(n_tensors, (float* const*)X_host, sums_host, "col_sums", t)) return st;
    col_sums_kernel<<<dim3((unsigned)ceil_div(cols, MASK_COLS), (unsigned)n_tensors), 256, 0, (hipStream_t)stream_>>>(t, N, cols, ldx);
    LLMREC_LAUNCH_CHECK();
    return LLMREC_OK;
}

int llmrec_mask_rows_f32(int32_t n_tensors, float* const* X_host, int64_t ldx, double* const* sums_host, int64_t N, int32_t cols,
                         const int64_t* nodes, int64_t m, llmrec_stream_t stream_) {
    MaskTensors t;
    LLMREC_CHECK_ARG(N >= 1 && cols >= 1 && ldx >= cols && m >= 0 && m <= N, "mask_rows: bad sizes");
    if (int st = mask_tensors(n_tensors, X_host, sums_host, "mask_rows", t)) return st;
    if (m == 0) return LLMREC_OK;
    LLMREC_CHECK_ARG(nodes, "mask_rows: null node list");
    mask_rows_kernel<<<dim3((unsigned)ceil_div(cols, MASK_COLS), (unsigned)n_tensors), 256, 0, (hipStream_t)stream_>>>(t, N, cols, ldx, nodes, m);
    LLMREC_LAUNCH_CHECK();
    return LLMREC_OK;
}

int llmrec_restore_loss_f32(int32_t n_streams, const float* const* X_host, int64_t ldx, const float* const* T_host, int64_t ldt,
                            float* const* dX_host, int64_t lddx, const int64_t* nodes, int64_t m, int32_t d, int32_t F,
                            const float* W, int64_t ldw, const float* b, int32_t loss_type, float alpha, float scale,
                            float* row_loss, float* loss_out, uint8_t* row_flags, const int32_t* row_stamp, llmrec_stream_t stream_) {
    LLMREC_CHECK_ARG(n_streams >= 1 && n_streams <= LLMREC_MASK_MAX_TENSORS, "restore_loss: %d streams outside [1, %d]", (int)n_streams,
                     LLMREC_MASK_MAX_TENSORS);
    LLMREC_CHECK_ARG(m >= 1 && m < (1ll << 31) && F >= 1 && d >= 1, "restore_loss: bad sizes (an empty node list has no mean)");
    LLMREC_CHECK_ARG(loss_type == LLMREC_RESTORE_SCE || loss_type == LLMREC_RESTORE_MSE, "restore_loss: loss_type %d", (int)loss_type);
    LLMREC_CHECK_ARG(alpha >= 1.f && alpha <= 64.f, "restore_loss: alpha = %g outside [1, 64]", (double)alpha);      // (false for a NaN)
    LLMREC_CHECK_ARG(X_host && T_host && nodes && W && b && row_loss && loss_out, "restore_loss: null pointer");
    LLMREC_CHECK_ARG((row_flags == nullptr) == (row_stamp == nullptr), "restore_loss: row_flags and row_stamp go together");
    LLMREC_CHECK_ARG(ldx >= d && ldt >= F && ldw >= d && (!dX_host || lddx >= d), "restore_loss: a leading dimension below its width");
    if (d != 64) { set_error("restore_loss: d = %d (compiled for 64)", (int)d); return LLMREC_EUNSUPPORTED; }
    RestoreArgs a = {};
    bool vx = ldx % 4 == 0, vt = ldt % 4 == 0, vd = lddx % 4 == 0;
    for (int i = 0; i < n_streams; ++i) {
        LLMREC_CHECK_ARG(X_host[i] && T_host[i] && (!dX_host || dX_host[i]), "restore_loss: stream %d: null pointer", i);
        LLMREC_CHECK_ARG((((uintptr_t)X_host[i] | (uintptr_t)T_host[i] | (uintptr_t)(dX_host ? dX_host[i] : nullptr)) & 3) == 0,
                         "restore_loss: stream %d: a base that is not 4-byte aligned", i);
        a.X[i] = X_host[i]; a.T[i] = T_host[i]; a.dX[i] = dX_host ? dX_host[i] : nullptr;
        vx = vx && ((uintptr_t)X_host[i] & 15) == 0; vt = vt && ((uintptr_t)T_host[i] & 15) == 0;
        vd = vd && dX_host && ((uintptr_t)dX_host[i] & 15) == 0;
    }
    LLMREC_CHECK_ARG((((uintptr_t)W | (uintptr_t)b) & 3) == 0, "restore_loss: W or b is not 4-byte aligned");
    a.ldx = ldx; a.ldt = ldt; a.lddx = lddx; a.ldw = ldw; a.m = m; a.nodes = nodes; a.W = W; a.b = b; a.F = F; a.loss_type = loss_type;
    a.vec_x = vx; a.vec_t = vt; a.vec_w = ldw % 4 == 0 && ((uintptr_t)W & 15) == 0; a.vec_dx = vd;
    a.alpha = alpha; a.scale = scale; a.row_loss = row_loss; a.row_flags = row_flags; a.row_stamp = row_stamp;
    const dim3 grid((unsigned)ceil_div(m, 64), (unsigned)n_streams);
    if (dX_host) restore_rows_kernel<true><<<grid, 256, 0, (hipStream_t)stream_>>>(a);
    else restore_rows_kernel<false><<<grid, 256, 0, (hipStream_t)stream_>>>(a);
    LLMREC_LAUNCH_CHECK();
    restore_reduce_kernel<<<1, 64 * n_streams, 0, (hipStream_t)stream_>>>(row_loss, m, loss_out);
    LLMREC_LAUNCH_CHECK();
    return LLMREC_OK;
}

int llmrec_restore_finish_f32(int32_t n_values, const float* values, float rate, float* scal4, double* running_sums3, int32_t n_views,
                              float* const* views_host, int64_t ld, int32_t cols, const int64_t* nodes, int64_t m, llmrec_stream_t stream_) {
    LLMREC_CHECK_ARG(n_values >= 0 && n_values <= 2 * LLMREC_MASK_MAX_TENSORS && (n_values == 0 || values), "restore_finish: bad values");
    LLMREC_CHECK_ARG(n_views >= 0 && n_views <= LLMREC_MASK_MAX_TENSORS && m >= 0, "restore_finish: bad views");
    FinishArgs a = {};
    const bool zero = n_views > 0 && m > 0;
    if (zero) {
        LLMREC_CHECK_ARG(views_host && nodes && cols >= 1 && ld >= cols, "restore_finish: null pointer or ld < cols");
        for (int i = 0; i < n_views; ++i) {
            LLMREC_CHECK_ARG(views_host[i] && ((uintptr_t)views_host[i] & 3) == 0, "restore_finish: view %d: null or misaligned", i);
            a.views[i] = views_host[i];
        }
    }
    if (!zero && n_values == 0) return LLMREC_OK;
    a.n_views = zero ? n_views : 0; a.cols = zero ? cols : 1; a.ld = ld; a.m = zero ? m : 0; a.nodes = nodes; a.values = values; a.n_values = n_values;
    a.rate = rate; a.scal = scal4; a.running = running_sums3;
    const int per = a.cols >= 256 ? 1 : 256 / a.cols;
    const int grid = 1 + (zero ? grid_for((int64_t)n_views * m, per) : 0);
    restore_finish_kernel<<<grid, 256, 0, (hipStream_t)stream_>>>(a);
    LLMREC_LAUNCH_CHECK();
    return LLMREC_OK;
}

}  // extern "C"
