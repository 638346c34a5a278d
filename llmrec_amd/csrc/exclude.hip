// exclude.hip - serving: exact masked top-K under PER-QUERY exclusion lists, with or without the item allow-list of serve.hip.
//
// The sweeps of topk.hip / topk_wide.hip take a mask CSR with ascending rows, and llmrec_score_topk_wide_f32 runs over a compact user table
// with an identity query list: a mask row belongs to a query. This file builds, on the device, mask row q = the ascending stable merge of
// (the train row of query_users[q]) and (exclusion row q, which arrives unsorted, with repeats and with padding), both in the numbering of
// the table that is swept - the compact numbering of an ItemFilter, or the item ids themselves without one - and hands it to the unchanged
// wide call. Not a line of the sweeps is involved.
//
// llmrec_score_topk_excluded_f32, on the caller's one stream:
//   ex_gather_users_kernel  the queried user rows as a compact [n_query][d4] table + the identity query list (as sf_gather_users_kernel of
//                           serve.hip); thread 0 opens the error word: with a filter, the host's n_kept against the device's count
//   ex_gather_items_kernel  filter only: the eligible rows of Ei as a dense [n_kept][d4] table (as sf_gather_items_kernel). Without a filter
//                           Ei is swept in place through ldi
//   ex_keys_kernel          entry e of exclusion row q -> the 64-bit key  q << 32 | id  (q by binary search in excl_rowptr; id in the swept
//                           numbering); an entry < 0, >= n_items or ineligible -> n_query << 32, which sorts behind every row. The same
//                           launch checks excl_rowptr: 0 at the front, excl_nnz at the back, non-decreasing - else the error word
//   (vendor radix sort)     the keys over bits [0, 32 + bits(n_query)), between two buffers of the workspace: rows in order, each ascending
//   ex_count_kernel         one wave per query: the kept entries of the train row (as sf_count_kernel), and where the query's keys begin
//                           (lower bound of q << 32 in the sorted keys; dropped keys lie behind, so the bound IS the exclusive scan of the kept
//                           exclusion counts)
//   ex_rowptr_kernel        one block: the train counts become the n_query + 1 row pointers of the train side, and those + the key bounds
//                           the row pointers of the merged mask; train entries beyond train_nnz, or the error word, zero both
//   ex_train_rows_kernel    one wave per query: the kept train entries in the swept numbering, in row order (as sf_mask_kernel)
//   ex_merge_kernel         one wave per query, wave-strided: a train entry lands at its index + the number of the query's keys BELOW it, a key
//                           at its index + the number of train entries AT OR BELOW it (binary searches; no LDS, no order carried from one
//                           round to the next): the stable ascending merge, duplicates kept on both sides, train entries first among equals
//   llmrec_score_topk_wide_f32 over the swept tables with the merged mask, capacity train_nnz + excl_nnz
//   ex_finish_kernel        with a filter: ids through old_id. Under the error word, with or without one: every entry -1 / -inf
// All sizes and launch counts come from host arguments; no allocation, no host read, no atomics (the error word is only ever set to 1, by plain
// stores behind the launch that opened it): capturable and deterministic.
#include "common.h"
#include <hipcub/hipcub.hpp>

namespace llmrec {

constexpr int EX_SCAN_THREADS = 1024;
constexpr int64_t EX_SORT_SLACK = 32ll << 20;                     // the bound llmrec_scatter_rows_workspace_bytes gives the same sort

__device__ __forceinline__ int ex_lanes_below(uint64_t mask, int lane) { return __popcll(mask & ((1ull << lane) - 1ull)); }

// the id of item c in the swept numbering, or -1: out of range, or ineligible under the filter
__device__ __forceinline__ int32_t ex_swept_id(const int32_t* __restrict__ new_id, int64_t n_items, int32_t c) {
    if (c < 0 || c >= n_items) return -1;
    return new_id ? new_id[c] : c;
}

// block = 256 >> shift rows x (1 << shift) columns (the power of two >= d4)
__global__ __launch_bounds__(256) void ex_gather_users_kernel(int n_query, const int64_t* __restrict__ query_users, const float* __restrict__ Eu, int64_t ldu,
                                                              int d, int d4, int shift, float* __restrict__ Ug, int64_t* __restrict__ ident,
                                                              const int32_t* __restrict__ n_kept_dev, int32_t n_kept, uint32_t* __restrict__ err) {
    const int k = threadIdx.x & ((1 << shift) - 1);
    const int64_t q = (int64_t)blockIdx.x * (256 >> shift) + (threadIdx.x >> shift);
    if (blockIdx.x == 0 && threadIdx.x == 0) *err = n_kept_dev && *n_kept_dev != n_kept ? 1u : 0u;
    if (q >= n_query || k >= d4) return;
    Ug[q * d4 + k] = k < d ? Eu[query_users[q] * ldu + k] : 0.0f;
    if (k == 0) ident[q] = q;
}

__global__ __launch_bounds__(256) void ex_gather_items_kernel(int32_t n_kept, const int32_t* __restrict__ old_id, const int32_t* __restrict__ n_kept_dev,
                                                              const float* __restrict__ Ei, int64_t ldi, int64_t n_items, int d, int d4, int shift,
                                                              float* __restrict__ Ig) {
    const int k = threadIdx.x & ((1 << shift) - 1);
    const int64_t r = (int64_t)blockIdx.x * (256 >> shift) + (threadIdx.x >> shift);
    if (r >= n_kept || k >= d4) return;
    float v = 0.0f;
    if (k < d && *n_kept_dev == n_kept) {                          // (a wrong n_kept: old_id may hold nothing at rank r)
        const int64_t old = old_id[r];
        if (old >= 0 && old < n_items) v = Ei[old * ldi + k];
    }
    Ig[r * d4 + k] = v;
}

// threads [0, n_query]: the checks of excl_rowptr; threads [0, excl_nnz): the keys. A broken excl_rowptr still gives every entry a row in
// [0, n_query) (the search never leaves the n_query + 1 pointers), and the error word empties the call.
__global__ __launch_bounds__(256) void ex_keys_kernel(int n_query, const int32_t* __restrict__ excl_rowptr, const int32_t* __restrict__ excl_colidx,
                                                      int64_t excl_nnz, const int32_t* __restrict__ new_id, int64_t n_items,
                                                      uint64_t* __restrict__ keys, uint32_t* __restrict__ err) {
    const int64_t work = excl_nnz > n_query + 1 ? excl_nnz : n_query + 1;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < work; e += (int64_t)gridDim.x * 256) {
        if (e <= n_query) {
            const int32_t here = excl_rowptr[e];
            const bool bad = e == n_query ? here != excl_nnz : (here > excl_rowptr[e + 1] || (e == 0 && here != 0));
            if (bad) *err = 1u;
        }
        if (e < excl_nnz) {
            int lo = 0, hi = n_query - 1;                          // the last row q with excl_rowptr[q] <= e
            while (lo < hi) {
                const int mid = lo + ((hi - lo + 1) >> 1);
                if (excl_rowptr[mid] <= e) lo = mid; else hi = mid - 1;
            }
            const int32_t id = ex_swept_id(new_id, n_items, excl_colidx[e]);
            keys[e] = id >= 0 ? ((uint64_t)lo << 32) | (uint32_t)id : (uint64_t)n_query << 32;
        }
    }
}

// waves [0, n_query]: wave q counts the kept entries of its train row (train side only) and finds where its keys begin; wave n_query finds
// where the kept keys end
__global__ __launch_bounds__(256) void ex_count_kernel(int n_query, const int64_t* __restrict__ query_users, const int32_t* __restrict__ train_rowptr,
                                                       const int32_t* __restrict__ train_colidx, const int32_t* __restrict__ new_id, int64_t n_items,
                                                       const uint64_t* __restrict__ keys, int64_t n_keys, int32_t* __restrict__ tcnt,
                                                       int32_t* __restrict__ kbeg) {
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q > n_query) return;                                       // (wave-uniform; the kernel has no block barrier)
    if (lane == 0) {
        const uint64_t head = (uint64_t)q << 32;
        int64_t lo = 0, hi = n_keys;
        while (lo < hi) { const int64_t mid = lo + ((hi - lo) >> 1); if (keys[mid] < head) lo = mid + 1; else hi = mid; }
        kbeg[q] = (int32_t)lo;
    }
    if (q == n_query || !train_rowptr) return;
    const int64_t u = query_users[q];
    const int32_t r0 = train_rowptr[u], r1 = train_rowptr[u + 1];
    int n = 0;
    for (int32_t base = r0; base < r1; base += 64) {
        const int32_t e = base + lane;
        n += __popcll(__ballot(e < r1 && ex_swept_id(new_id, n_items, train_colidx[e < r1 ? e : r0]) >= 0));
    }
    if (lane == 0) tcnt[q] = n;
}

// trp[0 .. n_query] = exclusive scan of tcnt (no train side: zeros), rp[q] = trp[q] + kbeg[q]; as sf_rowptr_kernel. A train total beyond
// cap_train or a set error word: zeros in both, and the word stays set
__global__ __launch_bounds__(EX_SCAN_THREADS) void ex_rowptr_kernel(int n_query, const int32_t* __restrict__ tcnt, const int32_t* __restrict__ kbeg,
                                                                    int64_t cap_train, int32_t* __restrict__ trp, int32_t* __restrict__ rp,
                                                                    uint32_t* __restrict__ err) {
    __shared__ int64_t wave_total[EX_SCAN_THREADS / 64];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const uint32_t was_bad = *err;                                 // (read by every thread before the barriers below; written once, after them)
    int64_t carry = 0;
    for (int64_t base = 0; base < n_query; base += EX_SCAN_THREADS) {
        const int64_t q = base + t;
        const int64_t len = q < n_query && tcnt ? tcnt[q] : 0;
        int64_t incl = len;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int64_t up = __shfl_up(incl, off, 64);
            if (lane >= off) incl += up;
        }
        if (lane == 63) wave_total[w] = incl;
        __syncthreads();
        int64_t before = 0, tile = 0;
#pragma unroll
        for (int i = 0; i < EX_SCAN_THREADS / 64; ++i) { const int64_t x = wave_total[i]; if (i < w) before += x; tile += x; }
        if (q < n_query) {
            const int64_t at = carry + before + incl - len;
            trp[q] = (int32_t)at;
            rp[q] = (int32_t)(at + kbeg[q]);
        }
        carry += tile;
        __syncthreads();                                           // (wave_total is rewritten by the next tile)
    }
    const bool bad = was_bad != 0u || carry > cap_train;
    if (bad)
        for (int64_t q = t; q < n_query; q += EX_SCAN_THREADS) { trp[q] = 0; rp[q] = 0; }
    if (t == 0) {
        trp[n_query] = bad ? 0 : (int32_t)carry;
        rp[n_query] = bad ? 0 : (int32_t)(carry + kbeg[n_query]);
        *err = bad ? 1u : 0u;
    }
}

__global__ __launch_bounds__(256) void ex_train_rows_kernel(int n_query, const int64_t* __restrict__ query_users, const int32_t* __restrict__ train_rowptr,
                                                            const int32_t* __restrict__ train_colidx, const int32_t* __restrict__ new_id, int64_t n_items,
                                                            const int32_t* __restrict__ trp, int32_t* __restrict__ tcol, int64_t cap_train,
                                                            const uint32_t* __restrict__ err) {
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= n_query || *err != 0u) return;                        // (wave-uniform; the kernel has no block barrier)
    const int64_t u = query_users[q];
    const int32_t r0 = train_rowptr[u], r1 = train_rowptr[u + 1];
    int64_t pos = trp[q];
    for (int32_t base = r0; base < r1; base += 64) {
        const int32_t e = base + lane;
        const int32_t id = e < r1 ? ex_swept_id(new_id, n_items, train_colidx[e]) : -1;
        const uint64_t m = __ballot(id >= 0);
        const int64_t at = pos + ex_lanes_below(m, lane);
        if (id >= 0 && at < cap_train) tcol[at] = id;
        pos += __popcll(m);
    }
}

// row q of the mask = the stable ascending merge of tcol[trp[q] .. trp[q + 1]) and the low words of keys[kbeg[q] .. kbeg[q + 1]). The lanes
// share nothing (no shuffle, no barrier): a lane's loops may end on their own.
__global__ __launch_bounds__(256) void ex_merge_kernel(int n_query, const int32_t* __restrict__ trp, const int32_t* __restrict__ tcol,
                                                       const int32_t* __restrict__ kbeg, const uint64_t* __restrict__ keys,
                                                       const int32_t* __restrict__ rp, int32_t* __restrict__ colidx, int64_t cap,
                                                       const uint32_t* __restrict__ err) {
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= n_query || *err != 0u) return;
    const int32_t a0 = trp[q], la = trp[q + 1] - a0;
    const int32_t b0 = kbeg[q], lb = kbeg[q + 1] - b0;
    const int64_t o0 = rp[q];
    for (int32_t i = lane; i < la; i += 64) {                      // a train entry: + the keys below it
        const int32_t a = tcol[a0 + i];
        int32_t lo = 0, hi = lb;
        while (lo < hi) { const int32_t mid = lo + ((hi - lo) >> 1); if ((int32_t)(uint32_t)keys[b0 + mid] < a) lo = mid + 1; else hi = mid; }
        const int64_t pos = o0 + i + lo;
        if (pos < cap) colidx[pos] = a;
    }
    for (int32_t j = lane; j < lb; j += 64) {                      // a key: + the train entries at or below it
        const int32_t b = (int32_t)(uint32_t)keys[b0 + j];
        int32_t lo = 0, hi = la;
        while (lo < hi) { const int32_t mid = lo + ((hi - lo) >> 1); if (tcol[a0 + mid] <= b) lo = mid + 1; else hi = mid; }
        const int64_t pos = o0 + j + lo;
        if (pos < cap) colidx[pos] = b;
    }
}

// old_id given: ids through it, -1 stays -1. Under the error word - or without one (err == nullptr: no eligible item, no sweep ran) - every
// entry becomes -1 / -inf
__global__ __launch_bounds__(256) void ex_finish_kernel(int64_t n, int64_t n_swept, const int32_t* __restrict__ old_id, int32_t* __restrict__ idx,
                                                        float* __restrict__ score, const uint32_t* __restrict__ err) {
    const bool bad = !err || *err != 0u;
    if (!bad && !old_id) return;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        const int32_t id = idx[e];
        if (bad || id < 0 || id >= n_swept) { idx[e] = -1; score[e] = -INFINITY; }
        else idx[e] = old_id[id];
    }
}

enum { EX_ITEMS, EX_USERS, EX_IDENT, EX_ERR, EX_TCNT, EX_TRP, EX_KBEG, EX_TCOL, EX_KEYS_A, EX_KEYS_B, EX_SORT, EX_RP, EX_COL, EX_PARTS };

// byte offsets, behind the wide call's workspace, of: item rows (filter only), user rows, query list, error word, train counts, train row
// pointers, key bounds, train columns, keys x 2, the sort's temporary storage, mask row pointers, mask columns; returns their total
static int64_t ex_parts(int32_t n_query, bool filtered, int32_t n_kept, int32_t d, int64_t train_nnz, int64_t excl_nnz, int64_t* off) {
    const int64_t n = n_query, d4 = align_up(d, 4), rp = align_up(4 * (n + 1), 256);
    off[EX_ITEMS] = 0;
    off[EX_USERS] = off[EX_ITEMS] + (filtered ? align_up(4 * (int64_t)n_kept * d4, 256) : 0);
    off[EX_IDENT] = off[EX_USERS] + align_up(4 * n * d4, 256);
    off[EX_ERR] = off[EX_IDENT] + align_up(8 * n, 256);
    off[EX_TCNT] = off[EX_ERR] + 256;
    off[EX_TRP] = off[EX_TCNT] + align_up(4 * n, 256);
    off[EX_KBEG] = off[EX_TRP] + rp;
    off[EX_TCOL] = off[EX_KBEG] + rp;
    off[EX_KEYS_A] = off[EX_TCOL] + align_up(4 * train_nnz, 256) + 256;
    off[EX_KEYS_B] = off[EX_KEYS_A] + align_up(8 * excl_nnz, 256);
    off[EX_SORT] = off[EX_KEYS_B] + align_up(8 * excl_nnz, 256);
    off[EX_RP] = off[EX_SORT] + (excl_nnz > 0 ? align_up(excl_nnz + EX_SORT_SLACK, 256) : 0);
    off[EX_COL] = off[EX_RP] + rp;
    return off[EX_COL] + align_up(4 * (train_nnz + excl_nnz), 256) + 256;   // (+ 256: every base lies inside the workspace at a count of 0 too)
}

static bool ex_sizes_ok(int32_t n_query, int64_t n_items, int32_t n_kept, int32_t d, int32_t K, int64_t train_nnz, int64_t excl_nnz) {
    return n_query >= 0 && n_items > 0 && n_items < (1ll << 31) && n_kept >= 0 && n_kept <= n_items && d > 0 && d <= 128 && K > 0 &&
           K <= LLMREC_TOPK_WIDE_MAX && train_nnz >= 0 && train_nnz < (1ll << 31) && excl_nnz >= 0 && excl_nnz < (1ll << 31) &&
           train_nnz + excl_nnz + (int64_t)n_query * K < (1ll << 31);
}

static int ex_shift(int d4) {
    int shift = 2;
    while ((1 << shift) < d4) ++shift;
    return shift;
}

// the key bits the sort must order: 32 of the id + those of n_query (the key of a dropped entry)
static int ex_end_bit(int32_t n_query) {
    int bits = 1;
    while (bits < 31 && ((int64_t)1 << bits) <= n_query) ++bits;
    return 32 + bits;
}

}  // namespace llmrec

using namespace llmrec;

extern "C" {

int64_t llmrec_score_topk_excluded_workspace_bytes(int32_t n_query, int64_t n_items, int32_t n_kept, int32_t d, int32_t K, int64_t train_nnz,
                                                   int64_t excl_nnz) {
    if (!ex_sizes_ok(n_query, n_items, n_kept, d, K, train_nnz, excl_nnz)) return -1;
    if (n_kept == 0) return 0;
    const int64_t wide = llmrec_score_topk_wide_workspace_bytes(n_query, n_kept, d, K, train_nnz + excl_nnz);
    if (wide < 0) return -1;
    int64_t off[EX_PARTS];
    return align_up(wide, 256) + ex_parts(n_query, n_kept != n_items, n_kept, d, train_nnz, excl_nnz, off);
}

int64_t llmrec_score_topk_excluded_mask_offset(int32_t n_query, int64_t n_items, int32_t n_kept, int32_t d, int32_t K, int64_t train_nnz,
                                               int64_t excl_nnz) {
    if (!ex_sizes_ok(n_query, n_items, n_kept, d, K, train_nnz, excl_nnz) || n_kept == 0) return -1;
    const int64_t wide = llmrec_score_topk_wide_workspace_bytes(n_query, n_kept, d, K, train_nnz + excl_nnz);
    if (wide < 0) return -1;
    int64_t off[EX_PARTS];
    ex_parts(n_query, n_kept != n_items, n_kept, d, train_nnz, excl_nnz, off);
    return align_up(wide, 256) + off[EX_RP];
}

int llmrec_score_topk_excluded_f32(int32_t n_query, const int64_t* query_users,
                                   const float* Eu, int64_t ldu, const float* Ei, int64_t ldi,
                                   int64_t n_items, int32_t d,
                                   const int32_t* train_rowptr, const int32_t* train_colidx,
                                   int32_t K, int32_t* out_idx, float* out_score,
                                   void* workspace, int64_t workspace_bytes, int32_t mode, int64_t train_nnz,
                                   const int32_t* excl_rowptr, const int32_t* excl_colidx, int64_t excl_nnz,
                                   const int32_t* new_id, const int32_t* old_id, const int32_t* n_kept_dev, int32_t n_kept,
                                   llmrec_stream_t stream_) {
    LLMREC_CHECK_ARG(n_query >= 0 && n_items > 0 && n_items < (1ll << 31) && d > 0 && K > 0 && K <= LLMREC_TOPK_WIDE_MAX,
                     "score_topk_excluded: bad sizes (K <= %d, n_items < 2^31)", LLMREC_TOPK_WIDE_MAX);
    LLMREC_CHECK_ARG(n_kept >= 0 && n_kept <= n_items, "score_topk_excluded: n_kept = %d outside [0, n_items]", n_kept);
    LLMREC_CHECK_ARG(mode == LLMREC_TOPK_MODE_EXACT_SWEEP || mode == LLMREC_TOPK_MODE_PREFILTER, "score_topk_excluded: unknown mode %d", mode);
    if (n_query == 0) return LLMREC_OK;
    LLMREC_CHECK_ARG(query_users && Eu && Ei && out_idx && out_score && ldu >= d && ldi >= d, "score_topk_excluded: null pointer or ld < d");
    const bool maps = new_id != nullptr;
    LLMREC_CHECK_ARG((old_id != nullptr) == maps && (n_kept_dev != nullptr) == maps,
                     "score_topk_excluded: the filter's maps are incomplete (all three, or none)");
    LLMREC_CHECK_ARG(maps || n_kept == n_items, "score_topk_excluded: no filter's maps, but n_kept = %d != n_items", n_kept);
    // a filter that keeps every item numbers the items as they are: Ei is swept in place, as without one (the count is still checked, and a
    // wrong one empties the call before a map would matter)
    const bool filtered = maps && n_kept != n_items;
    if (!filtered) new_id = nullptr;
    LLMREC_CHECK_ARG((train_rowptr == nullptr) == (train_colidx == nullptr), "score_topk_excluded: train CSR incomplete");
    LLMREC_CHECK_ARG(excl_nnz >= 0 && excl_nnz < (1ll << 31), "score_topk_excluded: excl_nnz outside [0, 2^31)");
    LLMREC_CHECK_ARG(excl_rowptr || excl_nnz == 0, "score_topk_excluded: excl_nnz > 0 without excl_rowptr");
    LLMREC_CHECK_ARG(excl_colidx || excl_nnz == 0, "score_topk_excluded: excl_nnz > 0 without excl_colidx");
    LLMREC_CHECK_EVAL_WIDTH(d);
    if (!train_rowptr) train_nnz = 0;
    LLMREC_CHECK_ARG(train_nnz >= 0 && train_nnz < (1ll << 31), "score_topk_excluded: train_nnz outside [0, 2^31)");
    const int64_t n_out = (int64_t)n_query * K;
    LLMREC_CHECK_ARG(train_nnz + excl_nnz + n_out < (1ll << 31), "score_topk_excluded: train_nnz + excl_nnz + n_query * K must lie in [0, 2^31)");
    hipStream_t stream = (hipStream_t)stream_;
    if (n_kept == 0) {                                             // no eligible item: every list is empty, no sweep is launched
        ex_finish_kernel<<<grid_for(n_out, 256), 256, 0, stream>>>(n_out, 0, nullptr, out_idx, out_score, nullptr);
        LLMREC_LAUNCH_CHECK();
        return LLMREC_OK;
    }
    const int64_t cap = train_nnz + excl_nnz;
    const int64_t wide = llmrec_score_topk_wide_workspace_bytes(n_query, n_kept, d, K, cap);
    LLMREC_CHECK_ARG(wide >= 0, "score_topk_excluded: the wide call refuses these sizes");
    int64_t off[EX_PARTS];
    const int64_t need = align_up(wide, 256) + ex_parts(n_query, filtered, n_kept, d, train_nnz, excl_nnz, off);
    LLMREC_CHECK_ARG(workspace && (uintptr_t)workspace % 16 == 0, "score_topk_excluded: needs the workspace (16-byte aligned)");
    if (workspace_bytes < need) {
        set_error("score_topk_excluded: workspace %lld < %lld", (long long)workspace_bytes, (long long)need);
        return LLMREC_EWORKSPACE;
    }
    char* x = (char*)workspace + align_up(wide, 256);
    float* Ig = (float*)(x + off[EX_ITEMS]);
    float* Ug = (float*)(x + off[EX_USERS]);
    int64_t* ident = (int64_t*)(x + off[EX_IDENT]);
    uint32_t* err = (uint32_t*)(x + off[EX_ERR]);
    int32_t* tcnt = (int32_t*)(x + off[EX_TCNT]);
    int32_t* trp = (int32_t*)(x + off[EX_TRP]);
    int32_t* kbeg = (int32_t*)(x + off[EX_KBEG]);
    int32_t* tcol = (int32_t*)(x + off[EX_TCOL]);
    uint64_t* keys_a = (uint64_t*)(x + off[EX_KEYS_A]);
    uint64_t* keys_b = (uint64_t*)(x + off[EX_KEYS_B]);
    void* temp = x + off[EX_SORT];
    int32_t* rp = (int32_t*)(x + off[EX_RP]);
    int32_t* colidx = (int32_t*)(x + off[EX_COL]);
    const int d4 = (int)align_up(d, 4), shift = ex_shift(d4);
    const int rows_per_block = 256 >> shift, wave_grid = (int)ceil_div(n_query, 4);

    hipcub::DoubleBuffer<uint64_t> kbuf(keys_a, keys_b);
    const int end_bit = ex_end_bit(n_query);
    size_t sort_need = 0;
    if (excl_nnz > 0) {                                            // (the query before the first launch)
        LLMREC_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, sort_need, kbuf, (int)excl_nnz, 0, end_bit, stream));
        if (sort_need > (size_t)align_up(excl_nnz + EX_SORT_SLACK, 256)) {
            set_error("score_topk_excluded: the sort needs %zu B of temporary storage > %lld", sort_need, (long long)align_up(excl_nnz + EX_SORT_SLACK, 256));
            return LLMREC_EWORKSPACE;
        }
    }
    ex_gather_users_kernel<<<(unsigned)ceil_div(n_query, rows_per_block), 256, 0, stream>>>(n_query, query_users, Eu, ldu, d, d4, shift, Ug, ident,
                                                                                             n_kept_dev, n_kept, err);
    LLMREC_LAUNCH_CHECK();
    if (filtered) {
        ex_gather_items_kernel<<<(unsigned)ceil_div(n_kept, rows_per_block), 256, 0, stream>>>(n_kept, old_id, n_kept_dev, Ei, ldi, n_items, d, d4, shift, Ig);
        LLMREC_LAUNCH_CHECK();
    }
    if (excl_rowptr) {
        const int64_t work = excl_nnz > (int64_t)n_query + 1 ? excl_nnz : (int64_t)n_query + 1;
        ex_keys_kernel<<<grid_for(work, 256), 256, 0, stream>>>(n_query, excl_rowptr, excl_colidx, excl_nnz, new_id, n_items, keys_a, err);
        LLMREC_LAUNCH_CHECK();
    }
    if (excl_nnz > 0) LLMREC_HIP(hipcub::DeviceRadixSort::SortKeys(temp, sort_need, kbuf, (int)excl_nnz, 0, end_bit, stream));
    const uint64_t* sorted = kbuf.Current();                       // (which buffer: settled on the host)
    ex_count_kernel<<<(unsigned)ceil_div((int64_t)n_query + 1, 4), 256, 0, stream>>>(n_query, query_users, train_rowptr, train_colidx, new_id, n_items,
                                                                                      sorted, excl_nnz, tcnt, kbeg);
    LLMREC_LAUNCH_CHECK();
    ex_rowptr_kernel<<<1, EX_SCAN_THREADS, 0, stream>>>(n_query, train_rowptr ? tcnt : nullptr, kbeg, train_nnz, trp, rp, err);
    LLMREC_LAUNCH_CHECK();
    if (train_rowptr) {
        ex_train_rows_kernel<<<wave_grid, 256, 0, stream>>>(n_query, query_users, train_rowptr, train_colidx, new_id, n_items, trp, tcol, train_nnz, err);
        LLMREC_LAUNCH_CHECK();
    }
    ex_merge_kernel<<<wave_grid, 256, 0, stream>>>(n_query, trp, tcol, kbeg, sorted, rp, colidx, cap, err);
    LLMREC_LAUNCH_CHECK();
    const int rc = llmrec_score_topk_wide_f32(n_query, ident, Ug, d4, filtered ? Ig : Ei, filtered ? d4 : ldi, n_kept, d, rp, colidx,
                                              K, out_idx, out_score, workspace, wide, mode, cap, stream_);
    if (rc != LLMREC_OK) return rc;
    ex_finish_kernel<<<grid_for(n_out, 256), 256, 0, stream>>>(n_out, n_kept, filtered ? old_id : nullptr, out_idx, out_score, err);
    LLMREC_LAUNCH_CHECK();
    return LLMREC_OK;
}

}  // extern "C"
