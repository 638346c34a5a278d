// serve.hip - serving: exact masked top-K under an item ALLOW-LIST and under PER-QUERY exclusion lists, by compaction in front of and behind
// the sweeps of topk.hip / topk_wide.hip.
//
// A score is a per-pair fma chain that does not depend on where a row sits, so ranking the eligible items alone is ranking a dense table of
// their rows, and a filter that keeps a tenth of the catalogue sweeps a tenth of it. The sweeps take a mask CSR with ascending rows, and
// llmrec_score_topk_wide_f32 runs over a compact user table with an identity query list: a mask row belongs to a query. ONE pipeline builds
// those tables and that mask for both scoring entries, in the numbering of the table that is swept - the compact numbering of an ItemFilter,
// or the item ids themselves without one - and hands them to the unchanged wide call. Not a line of the sweeps is involved.
//
// llmrec_item_filter_build: the id maps of an allow mask, an exclusive scan of the flags over blocks of LLMREC_FILTER_TILE items. Every
// cross-block hand-over is a kernel boundary (no block waits for another, no atomics):
//   if_count_kernel   block b: the number of non-zero flags of tile b
//   if_scan_kernel    one block: the counts become their exclusive scan, in place (block_exclusive_scan of compact.h); the total is n_kept
//   if_write_kernel   block b: rank of item i = (scan of tile b) + (flags before i inside the tile, by ballots); new_id[i] = rank or -1,
//                     old_id[rank] = i
// serve_pipeline, on the caller's one stream, for llmrec_score_topk_filtered_f32 (no merge: the mask is the train side alone) and
// llmrec_score_topk_excluded_f32 (merge: mask row q = the ascending stable merge of the train row of query_users[q] and exclusion row q):
//   sv_users_kernel       the queried user rows as a compact [n_query][d4] table + the identity query list (gather_user_rows of compact.h);
//                         thread 0 opens the error word: with a filter, the host's n_kept against the device's count - a difference sets the
//                         word for the rest of the call
//   sv_items_kernel       the eligible rows of Ei as a dense [n_kept][d4] table through old_id (64-bit row offsets, zero pad columns; zero
//                         rows under a wrong n_kept: old_id is then not read beyond what the build wrote). The filtered entry always runs it;
//                         the excluded entry sweeps Ei in place through ldi without a filter and under one that keeps every item
//   (merge) exclude_sorted_keys of exclude.hip: the keys kernel with an exclusion CSR, the vendor sort with excl_nnz > 0
//   sv_count_kernel       one wave per query: the entries c of the train row of query_users[q] that the swept table holds; merge: also where
//                         the query's keys begin (lower bound of q << 32 in the sorted keys; dropped keys lie behind, so the bound IS the
//                         exclusive scan of the kept exclusion counts)
//   sv_rowptr_kernel      one block: the train counts become the n_query + 1 row pointers of the train side; merge: those + the key bounds
//                         are the row pointers of the merged mask. Train entries beyond train_nnz, or the error word, zero them all
//   sv_train_rows_kernel  one wave per query: the kept train entries in the swept numbering, in row order (the map is monotone: ascending
//                         stays ascending, duplicates kept), positions by ballots. No merge: these rows ARE the mask
//   (merge) exclude_merge_rows of exclude.hip
//   llmrec_score_topk_wide_f32 over the swept tables with the mask, capacity train_nnz + excl_nnz
//   sv_finish_kernel      with a compact item table: ids through old_id, -1 stays -1. Under the error word every entry becomes -1 / -inf
// Without a train CSR the no-merge call skips count, row pointers and train rows (no mask at all); the merge call skips the train rows only.
// n_kept == 0 is one launch of sv_finish_kernel (every list empty: the sweeps refuse an empty table), n_query == 0 none.
// The error-word protocol exists once: sv_users_kernel opens it, sv_rowptr_kernel reads it before its barriers and writes it once after
// them, zeroes every row pointer under it, and no kernel writes a column beyond its capacity.
// All sizes and launch counts come from host arguments; no allocation, no host read, no atomics: capturable and deterministic.
#include "compact.h"

namespace llmrec {

constexpr int IF_THREADS = 256;
constexpr int IF_ROUNDS = LLMREC_FILTER_TILE / IF_THREADS;         // a thread owns items tile + j 256 + t: neighbouring lanes read neighbouring bytes
static_assert(LLMREC_FILTER_TILE % IF_THREADS == 0, "a tile is whole rounds of the block");

__global__ __launch_bounds__(IF_THREADS) void if_count_kernel(int64_t n_items, const uint8_t* __restrict__ allow, int32_t* __restrict__ block_cnt) {
    __shared__ int32_t wave_cnt[IF_THREADS / 64];
    const int t = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * LLMREC_FILTER_TILE;
    int n = 0;
#pragma unroll
    for (int j = 0; j < IF_ROUNDS; ++j) {
        const int64_t i = base + j * IF_THREADS + t;
        n += __popcll(__ballot(i < n_items && allow[i] != 0));     // (wave-uniform)
    }
    if ((t & 63) == 0) wave_cnt[t >> 6] = n;
    __syncthreads();
    if (t == 0) block_cnt[blockIdx.x] = (wave_cnt[0] + wave_cnt[1]) + (wave_cnt[2] + wave_cnt[3]);
}

// v[0 .. n) becomes its exclusive scan; *total = the sum (the total of the flags is below 2^31)
__global__ __launch_bounds__(SCAN_THREADS) void if_scan_kernel(int64_t n, int32_t* __restrict__ v, int32_t* __restrict__ total) {
    const int64_t sum = block_exclusive_scan<SCAN_THREADS>(n, [=](int64_t b) { return (int64_t)v[b]; }, [=](int64_t b, int64_t at) { v[b] = (int32_t)at; });
    if (threadIdx.x == 0) *total = (int32_t)sum;
}

__global__ __launch_bounds__(IF_THREADS) void if_write_kernel(int64_t n_items, const uint8_t* __restrict__ allow, const int32_t* __restrict__ block_off,
                                                              int32_t* __restrict__ new_id, int32_t* __restrict__ old_id) {
    __shared__ int32_t cnt[IF_ROUNDS][IF_THREADS / 64];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int64_t base = (int64_t)blockIdx.x * LLMREC_FILTER_TILE;
    uint32_t mine = 0u;                                            // bit j: my item of round j is eligible
    int below[IF_ROUNDS];                                          // eligible items of my wave's round j in the lanes below me (static indices only)
#pragma unroll
    for (int j = 0; j < IF_ROUNDS; ++j) {
        const int64_t i = base + j * IF_THREADS + t;
        const bool f = i < n_items && allow[i] != 0;
        const uint64_t m = __ballot(f);
        mine |= (f ? 1u : 0u) << j;
        below[j] = lanes_below(m, lane);
        if (lane == 0) cnt[j][w] = __popcll(m);
    }
    __syncthreads();
    int32_t running = block_off[blockIdx.x];
#pragma unroll
    for (int j = 0; j < IF_ROUNDS; ++j) {
        int32_t before = 0, round = 0;
#pragma unroll
        for (int x = 0; x < IF_THREADS / 64; ++x) { const int32_t c = cnt[j][x]; if (x < w) before += c; round += c; }
        const int64_t i = base + j * IF_THREADS + t;
        if (i < n_items) {
            const bool f = ((mine >> j) & 1u) != 0u;
            const int32_t rank = running + before + below[j];
            new_id[i] = f ? rank : -1;
            if (f) old_id[rank] = (int32_t)i;                      // (rank < the number of eligible items <= n_items)
        }
        running += round;
    }
}

__global__ __launch_bounds__(256) void sv_users_kernel(int n_query, const int64_t* __restrict__ query_users, const float* __restrict__ Eu, int64_t ldu,
                                                       int d, int d4, int shift, float* __restrict__ Ug, int64_t* __restrict__ ident,
                                                       const int32_t* __restrict__ n_kept_dev, int32_t n_kept, uint32_t* __restrict__ err) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *err = n_kept_dev && *n_kept_dev != n_kept ? 1u : 0u;
    gather_user_rows(n_query, query_users, Eu, ldu, d, d4, shift, Ug, ident, [](int64_t) {});
}

// block = 256 >> shift rows x (1 << shift) columns, as sv_users_kernel
__global__ __launch_bounds__(256) void sv_items_kernel(int32_t n_kept, const int32_t* __restrict__ old_id, const int32_t* __restrict__ n_kept_dev,
                                                       const float* __restrict__ Ei, int64_t ldi, int64_t n_items, int d, int d4, int shift,
                                                       float* __restrict__ Ig) {
    const int k = threadIdx.x & ((1 << shift) - 1);
    const int64_t r = (int64_t)blockIdx.x * (256 >> shift) + (threadIdx.x >> shift);
    if (r >= n_kept || k >= d4) return;                            // (the clamp to rank < n_kept)
    float v = 0.0f;
    if (k < d && *n_kept_dev == n_kept) {                          // (a wrong n_kept: old_id may hold nothing at rank r)
        const int64_t old = old_id[r];
        if (old >= 0 && old < n_items) v = Ei[old * ldi + k];
    }
    Ig[r * d4 + k] = v;
}

// waves [0, n_query): wave q counts the kept entries of its train row (train side only). kbeg given (merge): waves [0, n_query] find where
// the keys of query q begin, wave n_query where the kept keys end
__global__ __launch_bounds__(256) void sv_count_kernel(int n_query, const int64_t* __restrict__ query_users, const int32_t* __restrict__ train_rowptr,
                                                       const int32_t* __restrict__ train_colidx, const int32_t* __restrict__ new_id, int64_t n_items,
                                                       const uint64_t* __restrict__ keys, int64_t n_keys, int32_t* __restrict__ tcnt,
                                                       int32_t* __restrict__ kbeg) {
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q > n_query) return;                                       // (wave-uniform; the kernel has no block barrier)
    if (kbeg && lane == 0) {
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
        n += __popcll(__ballot(e < r1 && swept_id(new_id, n_items, train_colidx[e < r1 ? e : r0]) >= 0));
    }
    if (lane == 0) tcnt[q] = n;
}

// trp[0 .. n_query] = exclusive scan of tcnt (no train side: zeros); rp given (merge): rp[q] = trp[q] + kbeg[q]. A train total beyond
// cap_train or a set error word: zeros in both, and the word stays set
__global__ __launch_bounds__(SCAN_THREADS) void sv_rowptr_kernel(int n_query, const int32_t* __restrict__ tcnt, const int32_t* __restrict__ kbeg,
                                                                 int64_t cap_train, int32_t* __restrict__ trp, int32_t* __restrict__ rp,
                                                                 uint32_t* __restrict__ err) {
    const int t = threadIdx.x;
    const uint32_t was_bad = *err;                                 // (read by every thread before the scan's barriers; written once, after them)
    const int64_t total = block_exclusive_scan<SCAN_THREADS>(
        n_query, [=](int64_t q) { return (int64_t)(tcnt ? tcnt[q] : 0); },
        [=](int64_t q, int64_t at) {
            trp[q] = (int32_t)at;
            if (rp) rp[q] = (int32_t)(at + kbeg[q]);
        });
    const bool bad = was_bad != 0u || total > cap_train;
    if (bad)
        for (int64_t q = t; q < n_query; q += SCAN_THREADS) { trp[q] = 0; if (rp) rp[q] = 0; }
    if (t == 0) {
        trp[n_query] = bad ? 0 : (int32_t)total;
        if (rp) rp[n_query] = bad ? 0 : (int32_t)(total + kbeg[n_query]);
        *err = bad ? 1u : 0u;
    }
}

__global__ __launch_bounds__(256) void sv_train_rows_kernel(int n_query, const int64_t* __restrict__ query_users, const int32_t* __restrict__ train_rowptr,
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
        const int32_t id = e < r1 ? swept_id(new_id, n_items, train_colidx[e]) : -1;
        const uint64_t m = __ballot(id >= 0);
        const int64_t at = pos + lanes_below(m, lane);
        if (id >= 0 && at < cap_train) tcol[at] = id;
        pos += __popcll(m);
    }
}

// old_id given: ids through it, -1 stays -1. Under the error word - or without one (err == nullptr: no eligible item, no sweep ran) - every
// entry becomes -1 / -inf
__global__ __launch_bounds__(256) void sv_finish_kernel(int64_t n, int64_t n_swept, const int32_t* __restrict__ old_id, int32_t* __restrict__ idx,
                                                        float* __restrict__ score, const uint32_t* __restrict__ err) {
    const bool bad = !err || *err != 0u;
    if (!bad && !old_id) return;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        const int32_t id = idx[e];
        if (bad || id < 0 || id >= n_swept) { idx[e] = -1; score[e] = -INFINITY; }
        else idx[e] = old_id[id];
    }
}

enum { SV_ITEMS, SV_USERS, SV_IDENT, SV_ERR, SV_TCNT, SV_TRP, SV_KBEG, SV_TCOL, SV_KEYS_A, SV_KEYS_B, SV_SORT, SV_RP, SV_COL, SV_PARTS };

// byte offsets, behind the wide call's workspace, of: item rows (with a compact item table), user rows, query list, error word, train counts,
// train row pointers, train columns + 256 - the whole layout, and the mask, without a merge -, and with one: key bounds (in front of the
// train columns), keys x 2, the sort's temporary storage, mask row pointers, mask columns + 256; returns their total
// (+ 256: every base lies inside the workspace at a count of 0 too)
static int64_t sv_parts(bool merge, bool items, int32_t n_query, int32_t n_kept, int32_t d, int64_t train_nnz, int64_t excl_nnz, int64_t* off) {
    const int64_t n = n_query, d4 = align_up(d, 4), rp = align_up(4 * (n + 1), 256), keys = merge ? align_up(8 * excl_nnz, 256) : 0;
    off[SV_ITEMS] = 0;
    off[SV_USERS] = off[SV_ITEMS] + (items ? align_up(4 * (int64_t)n_kept * d4, 256) : 0);
    off[SV_IDENT] = off[SV_USERS] + align_up(4 * n * d4, 256);
    off[SV_ERR] = off[SV_IDENT] + align_up(8 * n, 256);
    off[SV_TCNT] = off[SV_ERR] + 256;
    off[SV_TRP] = off[SV_TCNT] + align_up(4 * n, 256);
    off[SV_KBEG] = off[SV_TRP] + rp;
    off[SV_TCOL] = off[SV_KBEG] + (merge ? rp : 0);
    off[SV_KEYS_A] = off[SV_TCOL] + align_up(4 * train_nnz, 256) + 256;
    off[SV_KEYS_B] = off[SV_KEYS_A] + keys;
    off[SV_SORT] = off[SV_KEYS_B] + keys;
    off[SV_RP] = off[SV_SORT] + (merge ? exclude_sort_reserve(excl_nnz) : 0);
    off[SV_COL] = off[SV_RP] + (merge ? rp : 0);
    return off[SV_COL] + (merge ? align_up(4 * (train_nnz + excl_nnz), 256) + 256 : 0);
}

// the excluded entry holds train_nnz + excl_nnz + n_query * K below 2^31 at every K; the filtered entry leaves its sum to the wide call (K > 64)
static bool sv_sizes_ok(bool merge, int32_t n_query, int64_t n_items, int32_t n_kept, int32_t d, int32_t K, int64_t train_nnz, int64_t excl_nnz) {
    return n_query >= 0 && n_items > 0 && n_items < (1ll << 31) && n_kept >= 0 && n_kept <= n_items && d > 0 && d <= 128 && K > 0 &&
           K <= LLMREC_TOPK_WIDE_MAX && train_nnz >= 0 && train_nnz < (1ll << 31) && excl_nnz >= 0 && excl_nnz < (1ll << 31) &&
           (!merge || train_nnz + excl_nnz + (int64_t)n_query * K < (1ll << 31));
}

// the workspace bytes of a call (-1: refused sizes; 0: no eligible item, no sweep) and the byte offset of its mask's row pointers (-1: none)
static int64_t sv_workspace_bytes(bool merge, int32_t n_query, int64_t n_items, int32_t n_kept, int32_t d, int32_t K, int64_t train_nnz, int64_t excl_nnz,
                                  int64_t* mask_offset) {
    *mask_offset = -1;
    if (!sv_sizes_ok(merge, n_query, n_items, n_kept, d, K, train_nnz, excl_nnz)) return -1;
    if (n_kept == 0) return 0;
    const int64_t wide = llmrec_score_topk_wide_workspace_bytes(n_query, n_kept, d, K, train_nnz + excl_nnz);
    if (wide < 0) return -1;
    int64_t off[SV_PARTS];
    const int64_t parts = sv_parts(merge, !merge || n_kept != n_items, n_query, n_kept, d, train_nnz, excl_nnz, off);
    *mask_offset = align_up(wide, 256) + off[merge ? SV_RP : SV_TRP];
    return align_up(wide, 256) + parts;
}

// one scoring call: the arguments of llmrec_score_topk_excluded_f32 (the filtered entry: no exclusion CSR), the entry's name for its messages
// and whether the exclusion stage runs
struct ServeCall {
    const char* name;
    bool merge;
    int32_t n_query;
    const int64_t* query_users;
    const float* Eu;
    int64_t ldu;
    const float* Ei;
    int64_t ldi, n_items;
    int32_t d;
    const int32_t *train_rowptr, *train_colidx;
    int32_t K;
    int32_t* out_idx;
    float* out_score;
    void* workspace;
    int64_t workspace_bytes;
    int32_t mode;
    int64_t train_nnz;
    const int32_t *excl_rowptr, *excl_colidx;
    int64_t excl_nnz;
    const int32_t *new_id, *old_id, *n_kept_dev;
    int32_t n_kept;
    llmrec_stream_t stream;
};

// the checks both entries share (an entry's own follow them); n_query == 0 passes before the pointers are looked at. Without a train CSR
// train_nnz becomes 0
static int sv_check_args(ServeCall& c) {
    LLMREC_CHECK_ARG(c.n_query >= 0 && c.n_items > 0 && c.n_items < (1ll << 31) && c.d > 0 && c.K > 0 && c.K <= LLMREC_TOPK_WIDE_MAX,
                     "%s: bad sizes (K <= %d, n_items < 2^31)", c.name, LLMREC_TOPK_WIDE_MAX);
    LLMREC_CHECK_ARG(c.n_kept >= 0 && c.n_kept <= c.n_items, "%s: n_kept = %d outside [0, n_items]", c.name, c.n_kept);
    LLMREC_CHECK_ARG(c.mode == LLMREC_TOPK_MODE_EXACT_SWEEP || c.mode == LLMREC_TOPK_MODE_PREFILTER, "%s: unknown mode %d", c.name, c.mode);
    if (c.n_query == 0) return LLMREC_OK;
    LLMREC_CHECK_ARG(c.query_users && c.Eu && c.Ei && c.out_idx && c.out_score && c.ldu >= c.d && c.ldi >= c.d, "%s: null pointer or ld < d", c.name);
    LLMREC_CHECK_ARG((c.train_rowptr == nullptr) == (c.train_colidx == nullptr), "%s: train CSR incomplete", c.name);
    LLMREC_CHECK_EVAL_WIDTH(c.d);
    if (!c.train_rowptr) c.train_nnz = 0;
    LLMREC_CHECK_ARG(c.train_nnz >= 0 && c.train_nnz < (1ll << 31), "%s: train_nnz outside [0, 2^31)", c.name);
    return LLMREC_OK;
}

// a checked call with n_query > 0
static int serve_pipeline(const ServeCall& c) {
    hipStream_t stream = (hipStream_t)c.stream;
    const int32_t n_query = c.n_query, n_kept = c.n_kept, d = c.d;
    const int64_t n_out = (int64_t)n_query * c.K, train_nnz = c.train_nnz, cap = train_nnz + c.excl_nnz;
    if (n_kept == 0) {                                             // no eligible item: every list is empty, no sweep is launched
        sv_finish_kernel<<<grid_for(n_out, 256), 256, 0, stream>>>(n_out, 0, nullptr, c.out_idx, c.out_score, nullptr);
        LLMREC_LAUNCH_CHECK();
        return LLMREC_OK;
    }
    // the excluded entry under a filter that keeps every item (or none given): the items are numbered as they are, Ei is swept in place (the
    // count is still checked, and a wrong one empties the call before a map would matter). The filtered entry always gathers
    const bool items = !c.merge || (c.new_id && n_kept != c.n_items);
    const int32_t *new_id = items ? c.new_id : nullptr, *old_id = items ? c.old_id : nullptr;
    const int64_t wide = llmrec_score_topk_wide_workspace_bytes(n_query, n_kept, d, c.K, cap);
    LLMREC_CHECK_ARG(wide >= 0, "%s: the wide call refuses these sizes (train_nnz + excl_nnz + n_query * K must lie in [0, 2^31))", c.name);
    int64_t off[SV_PARTS];
    const int64_t need = align_up(wide, 256) + sv_parts(c.merge, items, n_query, n_kept, d, train_nnz, c.excl_nnz, off);
    LLMREC_CHECK_ARG(c.workspace && (uintptr_t)c.workspace % 16 == 0, "%s: needs the workspace (16-byte aligned)", c.name);
    if (c.workspace_bytes < need) {
        set_error("%s: workspace %lld < %lld", c.name, (long long)c.workspace_bytes, (long long)need);
        return LLMREC_EWORKSPACE;
    }
    char* x = (char*)c.workspace + align_up(wide, 256);
    float* Ig = (float*)(x + off[SV_ITEMS]);
    float* Ug = (float*)(x + off[SV_USERS]);
    int64_t* ident = (int64_t*)(x + off[SV_IDENT]);
    uint32_t* err = (uint32_t*)(x + off[SV_ERR]);
    int32_t* tcnt = (int32_t*)(x + off[SV_TCNT]);
    int32_t* trp = (int32_t*)(x + off[SV_TRP]);
    int32_t* kbeg = c.merge ? (int32_t*)(x + off[SV_KBEG]) : nullptr;
    int32_t* tcol = (int32_t*)(x + off[SV_TCOL]);
    int32_t* rp = c.merge ? (int32_t*)(x + off[SV_RP]) : nullptr;
    int32_t* colidx = (int32_t*)(x + off[SV_COL]);
    const int d4 = (int)align_up(d, 4), shift = gather_shift(d4);
    const int rows_per_block = 256 >> shift, wave_grid = (int)ceil_div(n_query, 4);
    const bool train = c.train_rowptr != nullptr;
    int rc;

    size_t sort_need = 0;
    const uint64_t* sorted = nullptr;
    if (c.merge && (rc = exclude_sort_need(c.name, n_query, c.excl_nnz, &sort_need, stream)) != LLMREC_OK) return rc;   // (before the first launch)
    sv_users_kernel<<<(unsigned)ceil_div(n_query, rows_per_block), 256, 0, stream>>>(n_query, c.query_users, c.Eu, c.ldu, d, d4, shift, Ug, ident,
                                                                                      c.n_kept_dev, n_kept, err);
    LLMREC_LAUNCH_CHECK();
    if (items) {
        sv_items_kernel<<<(unsigned)ceil_div(n_kept, rows_per_block), 256, 0, stream>>>(n_kept, old_id, c.n_kept_dev, c.Ei, c.ldi, c.n_items, d, d4, shift, Ig);
        LLMREC_LAUNCH_CHECK();
    }
    if (c.merge && (rc = exclude_sorted_keys(n_query, c.excl_rowptr, c.excl_colidx, c.excl_nnz, new_id, c.n_items, (uint64_t*)(x + off[SV_KEYS_A]),
                                             (uint64_t*)(x + off[SV_KEYS_B]), x + off[SV_SORT], sort_need, err, &sorted, stream)) != LLMREC_OK)
        return rc;
    if (c.merge || train) {
        sv_count_kernel<<<(unsigned)ceil_div((int64_t)n_query + (c.merge ? 1 : 0), 4), 256, 0, stream>>>(n_query, c.query_users, c.train_rowptr, c.train_colidx,
                                                                                                         new_id, c.n_items, sorted, c.excl_nnz, tcnt, kbeg);
        LLMREC_LAUNCH_CHECK();
        sv_rowptr_kernel<<<1, SCAN_THREADS, 0, stream>>>(n_query, train ? tcnt : nullptr, kbeg, train_nnz, trp, rp, err);
        LLMREC_LAUNCH_CHECK();
    }
    if (train) {
        sv_train_rows_kernel<<<wave_grid, 256, 0, stream>>>(n_query, c.query_users, c.train_rowptr, c.train_colidx, new_id, c.n_items, trp, tcol, train_nnz, err);
        LLMREC_LAUNCH_CHECK();
    }
    if (c.merge && (rc = exclude_merge_rows(n_query, trp, tcol, kbeg, sorted, rp, colidx, cap, err, stream)) != LLMREC_OK) return rc;
    const bool mask = c.merge || train;                            // (no merge: the train rows are the mask)
    rc = llmrec_score_topk_wide_f32(n_query, ident, Ug, d4, items ? Ig : c.Ei, items ? d4 : c.ldi, n_kept, d, mask ? (c.merge ? rp : trp) : nullptr,
                                    mask ? (c.merge ? colidx : tcol) : nullptr, c.K, c.out_idx, c.out_score, c.workspace, wide, c.mode, cap, c.stream);
    if (rc != LLMREC_OK) return rc;
    sv_finish_kernel<<<grid_for(n_out, 256), 256, 0, stream>>>(n_out, n_kept, old_id, c.out_idx, c.out_score, err);
    LLMREC_LAUNCH_CHECK();
    return LLMREC_OK;
}

}  // namespace llmrec

using namespace llmrec;

extern "C" {

int64_t llmrec_item_filter_workspace_bytes(int64_t n_items) {
    if (n_items < 0 || n_items >= (1ll << 31)) return -1;
    return align_up(4 * ceil_div(n_items, LLMREC_FILTER_TILE), 256) + 256;
}

int llmrec_item_filter_build(int64_t n_items, const uint8_t* allow, int32_t* new_id, int32_t* old_id, int32_t* n_kept_dev,
                             void* workspace, int64_t workspace_bytes, llmrec_stream_t stream_) {
    LLMREC_CHECK_ARG(n_items >= 0 && n_items < (1ll << 31), "item_filter_build: n_items outside [0, 2^31)");
    LLMREC_CHECK_ARG(n_kept_dev && workspace && (n_items == 0 || (allow && new_id && old_id)), "item_filter_build: null pointer");
    if (workspace_bytes < llmrec_item_filter_workspace_bytes(n_items)) {
        set_error("item_filter_build: workspace %lld < %lld", (long long)workspace_bytes, (long long)llmrec_item_filter_workspace_bytes(n_items));
        return LLMREC_EWORKSPACE;
    }
    hipStream_t stream = (hipStream_t)stream_;
    const int64_t n_blocks = ceil_div(n_items, LLMREC_FILTER_TILE);
    int32_t* block_cnt = (int32_t*)workspace;
    if (n_blocks > 0) {
        if_count_kernel<<<(unsigned)n_blocks, IF_THREADS, 0, stream>>>(n_items, allow, block_cnt);
        LLMREC_LAUNCH_CHECK();
    }
    if_scan_kernel<<<1, SCAN_THREADS, 0, stream>>>(n_blocks, block_cnt, n_kept_dev);
    LLMREC_LAUNCH_CHECK();
    if (n_blocks > 0) {
        if_write_kernel<<<(unsigned)n_blocks, IF_THREADS, 0, stream>>>(n_items, allow, block_cnt, new_id, old_id);
        LLMREC_LAUNCH_CHECK();
    }
    return LLMREC_OK;
}

int64_t llmrec_score_topk_filtered_workspace_bytes(int32_t n_query, int64_t n_items, int32_t n_kept, int32_t d, int32_t K, int64_t train_nnz) {
    int64_t mask;
    return sv_workspace_bytes(false, n_query, n_items, n_kept, d, K, train_nnz, 0, &mask);
}

int64_t llmrec_score_topk_filtered_mask_offset(int32_t n_query, int64_t n_items, int32_t n_kept, int32_t d, int32_t K, int64_t train_nnz) {
    int64_t mask;
    sv_workspace_bytes(false, n_query, n_items, n_kept, d, K, train_nnz, 0, &mask);
    return mask;
}

int64_t llmrec_score_topk_excluded_workspace_bytes(int32_t n_query, int64_t n_items, int32_t n_kept, int32_t d, int32_t K, int64_t train_nnz,
                                                   int64_t excl_nnz) {
    int64_t mask;
    return sv_workspace_bytes(true, n_query, n_items, n_kept, d, K, train_nnz, excl_nnz, &mask);
}

int64_t llmrec_score_topk_excluded_mask_offset(int32_t n_query, int64_t n_items, int32_t n_kept, int32_t d, int32_t K, int64_t train_nnz,
                                               int64_t excl_nnz) {
    int64_t mask;
    sv_workspace_bytes(true, n_query, n_items, n_kept, d, K, train_nnz, excl_nnz, &mask);
    return mask;
}

int llmrec_score_topk_filtered_f32(int32_t n_query, const int64_t* query_users,
                                   const float* Eu, int64_t ldu, const float* Ei, int64_t ldi,
                                   int64_t n_items, int32_t d,
                                   const int32_t* train_rowptr, const int32_t* train_colidx,
                                   int32_t K, int32_t* out_idx, float* out_score,
                                   void* workspace, int64_t workspace_bytes, int32_t mode, int64_t train_nnz,
                                   const int32_t* new_id, const int32_t* old_id, const int32_t* n_kept_dev, int32_t n_kept,
                                   llmrec_stream_t stream_) {
    ServeCall c = {"score_topk_filtered", false, n_query, query_users, Eu, ldu, Ei, ldi, n_items, d, train_rowptr, train_colidx, K, out_idx, out_score,
                   workspace, workspace_bytes, mode, train_nnz, nullptr, nullptr, 0, new_id, old_id, n_kept_dev, n_kept, stream_};
    const int rc = sv_check_args(c);
    if (rc != LLMREC_OK || n_query == 0) return rc;
    LLMREC_CHECK_ARG(new_id && old_id && n_kept_dev, "score_topk_filtered: the filter's maps are missing");
    return serve_pipeline(c);
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
    ServeCall c = {"score_topk_excluded", true, n_query, query_users, Eu, ldu, Ei, ldi, n_items, d, train_rowptr, train_colidx, K, out_idx, out_score,
                   workspace, workspace_bytes, mode, train_nnz, excl_rowptr, excl_colidx, excl_nnz, new_id, old_id, n_kept_dev, n_kept, stream_};
    const int rc = sv_check_args(c);
    if (rc != LLMREC_OK || n_query == 0) return rc;
    const bool maps = new_id != nullptr;
    LLMREC_CHECK_ARG((old_id != nullptr) == maps && (n_kept_dev != nullptr) == maps,
                     "score_topk_excluded: the filter's maps are incomplete (all three, or none)");
    LLMREC_CHECK_ARG(maps || n_kept == n_items, "score_topk_excluded: no filter's maps, but n_kept = %d != n_items", n_kept);
    LLMREC_CHECK_ARG(excl_nnz >= 0 && excl_nnz < (1ll << 31), "score_topk_excluded: excl_nnz outside [0, 2^31)");
    LLMREC_CHECK_ARG(excl_rowptr || excl_nnz == 0, "score_topk_excluded: excl_nnz > 0 without excl_rowptr");
    LLMREC_CHECK_ARG(excl_colidx || excl_nnz == 0, "score_topk_excluded: excl_nnz > 0 without excl_colidx");
    LLMREC_CHECK_ARG(c.train_nnz + excl_nnz + (int64_t)n_query * K < (1ll << 31),
                     "score_topk_excluded: train_nnz + excl_nnz + n_query * K must lie in [0, 2^31)");
    return serve_pipeline(c);
}

}  // extern "C"
