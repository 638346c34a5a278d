// topk_wide.hip - R9/R10 beyond the 64 slots of a sweep: masked top-K for K <= LLMREC_TOPK_WIDE_MAX (1024) and the evaluation sums over such lists.
//
// ROUNDS over the sweeps of topk.hip. (score desc, item id asc) is a strict total order, so ranks [c p, c (p + 1)) of a user are exactly the
// top c of (candidates minus the user's first c p items). llmrec_score_topk_wide_f32 therefore calls llmrec_score_topk_mode_f32 ceil(K / c)
// times (c = 56 on the bf16 sweep, whose verification needs the spare slots; c = 64 on the exact sweep) and, before each pass, joins the items
// already emitted for a query to that query's mask row. Every pass is an ordinary masked top-K, proven exact by the call's own verification;
// not a line of the tuned sweeps is involved. What this file adds per call:
//   tw_gather_kernel   once: the queried user rows as a compact [n_query][d4] table + the identity query list. The mask CSR of the passes then
//                      has n_query + 1 row pointers whatever the user ids are (duplicate or unsorted query users get rows of their own), and
//                      copied row values give the same score bits.
//   tw_rowptr_kernel   per pass: row q's length = (previous generation's row q, the train row of the query's user in pass 0) + the valid ids
//                      of the last pass; one block scans them into the new row pointers (tiles of 1024 queries, int64 sums, fixed order). It also compares the
//                      total with the capacity the caller reserved: too small -> the overflow word is set for the rest of the call, the row
//                      pointers are zero (empty masks: nothing is written beyond a buffer) and every list comes back empty.
//   tw_merge_kernel    per pass: one wave per query. The <= 64 new ids are sorted across the lanes (bitonic, shuffles only); an entry of the
//                      old row lands at its index + (new ids below it), a new id at its index + (old entries <= it): the stable ascending
//                      merge the sweeps' cursors need, duplicates of the train row kept. Entries < 0 (exhausted users) are never merged.
//   tw_scatter_kernel  per pass: the pass's kp columns into columns [off, off + kp) of the [n_query][K] outputs, and the number of valid ids
//                      per query for the next pass's scan.
// Two generations of row pointers and columns alternate (a pass reads the previous one while it writes its own). All launch counts and
// sizes come from host arguments; no atomics, no allocation, nothing read back: capturable and deterministic.
//
// tw_eval_sums_kernel: llmrec_topk_eval_sums for 128 < K <= 1024. The one-thread-per-user kernel of topk.hip keeps its hit flags in two 64-bit
// words; here a WAVE owns a user: lane l tests ranks l, l + 64, ... (one bit per rank in a lane-private word, statically indexed), the sums
// over the ranks are lane-partial + butterfly, and a block adds its 128 users in a fixed order (wave w: users 32 w .. 32 w + 31 one after the
// other; then the four waves pairwise) into the partial layout of the one-thread kernel: llmrec_topk_eval_sums (topk.hip) launches this kernel
// through topk_eval_sums_wide_partials and adds the partials with its own second launch.
#include "compact.h"
#include <limits.h>

namespace llmrec {

constexpr int TW_MAX_RANK_WORDS = LLMREC_TOPK_WIDE_MAX / 64;      // 16 ranks per lane

// gather_user_rows (compact.h) + what the rounds start from: no ids emitted yet, the overflow word open
__global__ __launch_bounds__(256) void tw_gather_kernel(int n_query, const int64_t* __restrict__ query_users, const float* __restrict__ Eu, int64_t ldu,
                                                        int d, int d4, int shift, float* __restrict__ Ug, int64_t* __restrict__ ident,
                                                        int32_t* __restrict__ cnt, uint32_t* __restrict__ ovf) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *ovf = 0u;
    gather_user_rows(n_query, query_users, Eu, ldu, d, d4, shift, Ug, ident, [=](int64_t q) { cnt[q] = 0; });
}

__device__ __forceinline__ int64_t tw_row_len(const int32_t* __restrict__ a_rowptr, const int64_t* __restrict__ a_rows, const int32_t* __restrict__ cnt, int64_t q) {
    int64_t len = cnt[q];
    if (a_rowptr) { const int64_t r = a_rows ? a_rows[q] : q; len += a_rowptr[r + 1] - a_rowptr[r]; }
    return len;
}

// rowptr[0 .. n_query] = exclusive scan of the new row lengths (block_exclusive_scan of compact.h). When the total exceeds the capacity the
// row pointers are overwritten with zeros.
__global__ __launch_bounds__(SCAN_THREADS) void tw_rowptr_kernel(int n_query, const int32_t* __restrict__ a_rowptr, const int64_t* __restrict__ a_rows,
                                                                 const int32_t* __restrict__ cnt, int64_t cap, int32_t* __restrict__ rowptr,
                                                                 uint32_t* __restrict__ ovf) {
    const int t = threadIdx.x;
    const uint32_t was_bad = *ovf;                                 // (read by every thread before the scan's barriers; written once, after them)
    const int64_t total = block_exclusive_scan<SCAN_THREADS>(
        n_query, [=](int64_t q) { return tw_row_len(a_rowptr, a_rows, cnt, q); }, [=](int64_t q, int64_t at) { rowptr[q] = (int32_t)at; });
    const bool bad = was_bad != 0u || total > cap;
    if (bad)
        for (int64_t q = t; q < n_query; q += SCAN_THREADS) rowptr[q] = 0;
    if (t == 0) { rowptr[n_query] = bad ? 0 : (int32_t)total; *ovf = bad ? 1u : 0u; }
}

__global__ __launch_bounds__(256) void tw_merge_kernel(int n_query, const int32_t* __restrict__ a_rowptr, const int32_t* __restrict__ a_colidx,
                                                       const int64_t* __restrict__ a_rows, const int32_t* __restrict__ new_idx, int kp,
                                                       const int32_t* __restrict__ rowptr, int32_t* __restrict__ colidx, int64_t cap,
                                                       const uint32_t* __restrict__ ovf) {
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= n_query || *ovf != 0u) return;                        // (wave-uniform; the kernel has no block barrier)
    int32_t a0 = 0, a1 = 0;
    if (a_rowptr) { const int64_t r = a_rows ? a_rows[q] : q; a0 = a_rowptr[r]; a1 = a_rowptr[r + 1]; }
    const int la = a1 - a0;
    int32_t v = INT_MAX;                                           // the new ids, one per lane; INT_MAX = none (sorts behind every id)
    if (lane < kp) { const int32_t id = new_idx[q * kp + lane]; if (id >= 0) v = id; }
    const int nb = __popcll(__ballot(v != INT_MAX));
#pragma unroll
    for (int k = 2; k <= 64; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
            const int32_t o = __shfl_xor(v, j, 64);
            const bool keep_min = ((lane & j) == 0) == ((lane & k) == 0);
            v = keep_min ? (v < o ? v : o) : (v > o ? v : o);
        }
    }
    const int64_t o0 = rowptr[q];
    // old entries: index + the number of new ids below the entry (every lane runs the seven steps: the shuffles read all 64 lanes)
    for (int base = 0; base < la; base += 64) {
        const int i = base + lane;
        const bool active = i < la;
        const int32_t a = active ? a_colidx[a0 + i] : 0;
        int lo = 0, hi = nb;
#pragma unroll
        for (int step = 0; step < 7; ++step) {
            const int mid = (lo + hi) >> 1;
            const int32_t bm = __shfl(v, mid & 63, 64);
            if (lo < hi) { if (bm < a) lo = mid + 1; else hi = mid; }
        }
        const int64_t pos = o0 + i + lo;
        if (active && pos < cap) colidx[pos] = a;
    }
    // new ids: index + the number of old entries <= the id
    if (lane < nb) {
        int32_t lo = a0, hi = a1;
        while (lo < hi) { const int32_t mid = lo + ((hi - lo) >> 1); if (a_colidx[mid] <= v) lo = mid + 1; else hi = mid; }
        const int64_t pos = o0 + lane + (lo - a0);
        if (pos < cap) colidx[pos] = v;
    }
}

__global__ __launch_bounds__(256) void tw_scatter_kernel(int n_query, int kp, const int32_t* __restrict__ tmp_idx, const float* __restrict__ tmp_score,
                                                         int K, int off, int32_t* __restrict__ out_idx, float* __restrict__ out_score,
                                                         int32_t* __restrict__ cnt, const uint32_t* __restrict__ ovf) {
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= n_query) return;
    const bool bad = *ovf != 0u;
    int32_t id = -1;
    float s = -INFINITY;
    if (lane < kp && !bad) { id = tmp_idx[q * kp + lane]; s = tmp_score[q * kp + lane]; }
    if (lane < kp) { out_idx[q * K + off + lane] = id; out_score[q * K + off + lane] = s; }
    const int n = __popcll(__ballot(id >= 0));
    if (lane == 0) cnt[q] = n;
}

struct WideKs { int32_t k[8]; int32_t n; };
constexpr int TW_ES_USERS = 128;                                   // users per block: the partial layout of llmrec_topk_eval_sums_workspace_bytes

template <typename T>
__device__ __forceinline__ T tw_wave_sum(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__global__ __launch_bounds__(256) void tw_eval_sums_kernel(int n_query, const int64_t* __restrict__ query_users, int K, const int32_t* __restrict__ topk_idx,
                                                           const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx, WideKs ks,
                                                           double* __restrict__ partial) {
    __shared__ double red[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int nv = 4 * ks.n;
    double acc[4][8];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int t = 0; t < 8; ++t) acc[m][t] = 0.0;
    for (int i = 0; i < TW_ES_USERS / 4; ++i) {
        const int64_t q = (int64_t)blockIdx.x * TW_ES_USERS + w * (TW_ES_USERS / 4) + i;
        if (q >= n_query) break;                                   // (wave-uniform)
        const int64_t u = query_users[q];
        const int32_t r0 = rowptr[u], r1 = rowptr[u + 1];
        const double n_pos = (double)(r1 - r0);
        const int32_t* id = topk_idx + q * K;
        uint32_t mine = 0u;                                        // bit r: rank 64 r + lane is a hit
        int my_hits = 0, my_len = 0;
#pragma unroll
        for (int r = 0; r < TW_MAX_RANK_WORDS; ++r) {
            if (r * 64 >= K) break;                                // (uniform)
            const int j = r * 64 + lane;
            const int32_t item = j < K ? id[j] : -1;
            int32_t lo = r0, hi = r1;
            while (lo < hi) { const int32_t mid = lo + ((hi - lo) >> 1); if (colidx[mid] < item) lo = mid + 1; else hi = mid; }
            const bool h = item >= 0 && lo < r1 && colidx[lo] == item;
            mine |= (h ? 1u : 0u) << r;
            my_hits += h; my_len += item >= 0;
        }
        const int total_hits = tw_wave_sum(my_hits), list_len = tw_wave_sum(my_len);
        int s[8];
        double dcg[8], idcg[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) { s[t] = 0; dcg[t] = 0.0; idcg[t] = 0.0; }
#pragma unroll
        for (int r = 0; r < TW_MAX_RANK_WORDS; ++r) {
            if (r * 64 >= K) break;                                // (uniform)
            const int j = r * 64 + lane;
            if (j < K) {
                const double disc = 1.0 / log2((double)(j + 2));
                const bool h = ((mine >> r) & 1u) != 0u;
#pragma unroll
                for (int t = 0; t < 8; ++t) {
                    if (t < ks.n && j < ks.k[t]) {
                        if (h) { s[t] += 1; dcg[t] += disc; }
                        if (j < total_hits) idcg[t] += disc;
                    }
                }
            }
        }
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            if (t < ks.n) {                                        // (uniform)
                const int kk = ks.k[t] < K ? ks.k[t] : K;
                const double st = (double)tw_wave_sum(s[t]), d1 = tw_wave_sum(dcg[t]), d2 = tw_wave_sum(idcg[t]);
                const int denom = list_len < kk ? list_len : kk;
                acc[0][t] += st / (double)(denom > 0 ? denom : 1);
                acc[1][t] += n_pos > 0.0 ? st / n_pos : 0.0;
                acc[2][t] += d2 > 0.0 ? d1 / d2 : 0.0;
                acc[3][t] += st > 0.0 ? 1.0 : 0.0;
            }
        }
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) {
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            if (t < ks.n) {                                        // (block-uniform)
                if (lane == 0) red[w] = acc[m][t];
                __syncthreads();
                if (threadIdx.x == 0) partial[(int64_t)blockIdx.x * nv + m * ks.n + t] = (red[0] + red[1]) + (red[2] + red[3]);
                __syncthreads();
            }
        }
    }
}

// byte offsets, behind the single-sweep workspace, of: user rows, query list, row pointers x 2, counts, overflow word, columns x 2, pass ids,
// pass scores; returns their total
static int64_t tw_extra_parts(int32_t n_query, int32_t d, int32_t K, int64_t train_nnz, int64_t* off) {
    const int64_t n = n_query, d4 = align_up(d, 4), cols = align_up(4 * (train_nnz + n * K), 256), rp = align_up(4 * (n + 1), 256),
                  pass = align_up(4 * LLMREC_TOPK_MAX * n, 256);
    off[0] = 0;
    off[1] = off[0] + align_up(4 * n * d4, 256);
    off[2] = off[1] + align_up(8 * n, 256);
    off[3] = off[2] + rp;
    off[4] = off[3] + rp;
    off[5] = off[4] + align_up(4 * n, 256);
    off[6] = off[5] + 256;
    off[7] = off[6] + cols;
    off[8] = off[7] + cols;
    off[9] = off[8] + pass;
    return off[9] + pass;
}

// the first launch of llmrec_topk_eval_sums (csrc/topk.hip, which has checked the arguments and adds the partials) for lists beyond 128 columns
int topk_eval_sums_wide_partials(int32_t n_query, const int64_t* query_users, int32_t K, const int32_t* topk_idx, const int32_t* rowptr,
                                 const int32_t* colidx, int32_t n_ks, const int32_t* ks_host, double* partial, hipStream_t stream) {
    WideKs ks = {};
    ks.n = n_ks;
    for (int i = 0; i < n_ks; ++i) ks.k[i] = ks_host[i];
    const int n_blocks = (int)ceil_div(n_query, TW_ES_USERS);
    if (n_blocks > 0) {
        tw_eval_sums_kernel<<<n_blocks, 256, 0, stream>>>(n_query, query_users, K, topk_idx, rowptr, colidx, ks, partial);
        LLMREC_LAUNCH_CHECK();
    }
    return LLMREC_OK;
}

}  // namespace llmrec

using namespace llmrec;

extern "C" {

int64_t llmrec_score_topk_wide_workspace_bytes(int32_t n_query, int64_t n_items, int32_t d, int32_t K, int64_t train_nnz) {
    if (n_query < 0 || n_items <= 0 || d <= 0 || K <= 0 || K > LLMREC_TOPK_WIDE_MAX || train_nnz < 0) return -1;
    const int64_t base = llmrec_score_topk_workspace_bytes(n_query, n_items, d);
    if (base < 0 || K <= LLMREC_TOPK_MAX) return base;
    if (train_nnz + (int64_t)n_query * K >= (1ll << 31)) return -1;
    int64_t off[10];
    return align_up(base, 256) + tw_extra_parts(n_query, d, K, train_nnz, off);
}

int llmrec_score_topk_wide_f32(int32_t n_query, const int64_t* query_users,
                               const float* Eu, int64_t ldu, const float* Ei, int64_t ldi,
                               int64_t n_items, int32_t d,
                               const int32_t* train_rowptr, const int32_t* train_colidx,
                               int32_t K, int32_t* out_idx, float* out_score,
                               void* workspace, int64_t workspace_bytes, int32_t mode, int64_t train_nnz, llmrec_stream_t stream_) {
    LLMREC_CHECK_ARG(n_query >= 0 && n_items > 0 && d > 0 && K > 0 && K <= LLMREC_TOPK_WIDE_MAX, "score_topk_wide: bad sizes (K <= %d)", LLMREC_TOPK_WIDE_MAX);
    LLMREC_CHECK_ARG(mode == LLMREC_TOPK_MODE_EXACT_SWEEP || mode == LLMREC_TOPK_MODE_PREFILTER, "score_topk_wide: unknown mode %d", mode);
    if (n_query == 0) return LLMREC_OK;
    LLMREC_CHECK_ARG(query_users && Eu && Ei && out_idx && out_score && ldu >= d && ldi >= d, "score_topk_wide: null pointer or ld < d");
    LLMREC_CHECK_ARG((train_rowptr == nullptr) == (train_colidx == nullptr), "score_topk_wide: train CSR incomplete");
    LLMREC_CHECK_ARG(n_items < (1ll << 31), "score_topk_wide: n_items exceeds int32 item ids");
    LLMREC_CHECK_EVAL_WIDTH(d);                                // (before the gather and the mask launches of the rounds)
    if (workspace) {
        const int64_t need = llmrec_score_topk_wide_workspace_bytes(n_query, n_items, d, K, K > LLMREC_TOPK_MAX && train_nnz > 0 ? train_nnz : 0);
        if (need >= 0 && workspace_bytes < need) {
            set_error("score_topk_wide: workspace %lld < %lld", (long long)workspace_bytes, (long long)need);
            return LLMREC_EWORKSPACE;
        }
    }
    if (K <= LLMREC_TOPK_MAX)
        return llmrec_score_topk_mode_f32(n_query, query_users, Eu, ldu, Ei, ldi, n_items, d, train_rowptr, train_colidx, K, out_idx, out_score,
                                          workspace, workspace_bytes, mode, stream_);
    LLMREC_CHECK_ARG(train_nnz >= 0 && train_nnz + (int64_t)n_query * K < (1ll << 31), "score_topk_wide: train_nnz + n_query * K must lie in [0, 2^31)");
    LLMREC_CHECK_ARG(workspace && (uintptr_t)workspace % 16 == 0, "score_topk_wide: K > %d needs the workspace (16-byte aligned)", LLMREC_TOPK_MAX);
    hipStream_t stream = (hipStream_t)stream_;
    const int64_t base = llmrec_score_topk_workspace_bytes(n_query, n_items, d);
    int64_t off[10];
    tw_extra_parts(n_query, d, K, train_nnz, off);
    char* x = (char*)workspace + align_up(base, 256);
    float* Ug = (float*)(x + off[0]);
    int64_t* ident = (int64_t*)(x + off[1]);
    int32_t* rp[2] = {(int32_t*)(x + off[2]), (int32_t*)(x + off[3])};
    int32_t* cnt = (int32_t*)(x + off[4]);
    uint32_t* ovf = (uint32_t*)(x + off[5]);
    int32_t* ci[2] = {(int32_t*)(x + off[6]), (int32_t*)(x + off[7])};
    int32_t* tmp_idx = (int32_t*)(x + off[8]);
    float* tmp_score = (float*)(x + off[9]);
    const int d4 = (int)align_up(d, 4);
    const int64_t cap = train_nnz + (int64_t)n_query * K;
    const int c = mode == LLMREC_TOPK_MODE_PREFILTER ? LLMREC_TOPK_PREFILTER_MAX_K : LLMREC_TOPK_MAX;
    const int wave_grid = (int)ceil_div(n_query, 4);

    const int shift = gather_shift(d4);
    LLMREC_CHECK_ARG(shift <= 8, "score_topk_wide: d = %d > 256", d);
    tw_gather_kernel<<<(unsigned)ceil_div(n_query, 256 >> shift), 256, 0, stream>>>(n_query, query_users, Eu, ldu, d, d4, shift, Ug, ident, cnt, ovf);
    LLMREC_LAUNCH_CHECK();
    int p = 0;
    for (int col = 0; col < K; col += c, ++p) {
        const int kp = K - col < c ? K - col : c;
        // the mask of this pass: the previous generation (pass 0: the train rows of the queried users) + the ids of the last pass
        const int32_t* a_rowptr = p == 0 ? train_rowptr : rp[(p - 1) & 1];
        const int32_t* a_colidx = p == 0 ? train_colidx : ci[(p - 1) & 1];
        const int64_t* a_rows = p == 0 ? query_users : nullptr;
        tw_rowptr_kernel<<<1, SCAN_THREADS, 0, stream>>>(n_query, a_rowptr, a_rows, cnt, train_nnz + (int64_t)n_query * col, rp[p & 1], ovf);   // (pass 0: the train rows alone against train_nnz)
        LLMREC_LAUNCH_CHECK();
        tw_merge_kernel<<<wave_grid, 256, 0, stream>>>(n_query, a_rowptr, a_colidx, a_rows, tmp_idx, p == 0 ? 0 : c, rp[p & 1], ci[p & 1], cap, ovf);
        LLMREC_LAUNCH_CHECK();
        const int rc = llmrec_score_topk_mode_f32(n_query, ident, Ug, d4, Ei, ldi, n_items, d, rp[p & 1], ci[p & 1], kp, tmp_idx, tmp_score,
                                                  workspace, base, mode, stream_);
        if (rc != LLMREC_OK) return rc;
        tw_scatter_kernel<<<wave_grid, 256, 0, stream>>>(n_query, kp, tmp_idx, tmp_score, K, col, out_idx, out_score, cnt, ovf);
        LLMREC_LAUNCH_CHECK();
    }
    return LLMREC_OK;
}

}  // extern "C"
