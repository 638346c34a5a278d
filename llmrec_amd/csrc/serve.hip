// serve.hip - serving: exact masked top-K under an item ALLOW-LIST, by compaction in front of and behind the sweeps of topk.hip / topk_wide.hip.
//
// A score is a per-pair fma chain that does not depend on where a row sits, so ranking the eligible items alone is ranking a dense table of
// their rows: not a line of the tuned sweeps is involved, and a filter that keeps a tenth of the catalogue sweeps a tenth of it.
//
// llmrec_item_filter_build: the id maps of an allow mask, an exclusive scan of the flags over blocks of LLMREC_FILTER_TILE items. Every
// cross-block hand-over is a kernel boundary (no block waits for another, no atomics):
//   if_count_kernel   block b: the number of non-zero flags of tile b
//   if_scan_kernel    one block: the counts become their exclusive scan, in place (tiles of 1024 counts, as tw_rowptr_kernel); the total is n_kept
//   if_write_kernel   block b: rank of item i = (scan of tile b) + (flags before i inside the tile, by ballots); new_id[i] = rank or -1,
//                     old_id[rank] = i
// llmrec_score_topk_filtered_f32, on the caller's one stream:
//   sf_gather_users_kernel  the queried user rows as a compact [n_query][d4] table + the identity query list (as tw_gather_kernel); thread 0
//                           compares the host's n_kept with the device's count: a difference sets the error word for the rest of the call
//   sf_gather_items_kernel  the eligible rows of Ei as a dense [n_kept][d4] table through old_id (64-bit row offsets, zero pad columns; zero
//                           rows under a wrong n_kept: old_id is then not read beyond what the build wrote)
//   sf_count_kernel         one wave per query: the entries c of the train row of query_users[q] with new_id[c] >= 0
//   sf_rowptr_kernel        one block: the counts become n_query + 1 row pointers; a total beyond train_nnz, or the error word, zeroes them
//   sf_mask_kernel          one wave per query: the kept entries in row order as new_id[c] (the map is monotone: ascending stays ascending,
//                           duplicates kept), positions by ballots
//   llmrec_score_topk_wide_f32 on the compact tables with the mask as its train CSR
//   sf_map_back_kernel      ids through old_id, -1 stays -1; under the error word every entry becomes -1 / -inf
// All sizes and launch counts come from host arguments; no allocation, no host read, no atomics: capturable and deterministic.
#include "common.h"

namespace llmrec {

constexpr int IF_THREADS = 256;
constexpr int IF_ROUNDS = LLMREC_FILTER_TILE / IF_THREADS;         // a thread owns items tile + j 256 + t: neighbouring lanes read neighbouring bytes
constexpr int SF_SCAN_THREADS = 1024;
static_assert(LLMREC_FILTER_TILE % IF_THREADS == 0, "a tile is whole rounds of the block");

__device__ __forceinline__ int lanes_below(uint64_t mask, int lane) { return __popcll(mask & ((1ull << lane) - 1ull)); }

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

// v[0 .. n) becomes its exclusive scan; *total = the sum (int64 carries in a fixed order; the total of the flags is below 2^31)
__global__ __launch_bounds__(SF_SCAN_THREADS) void if_scan_kernel(int64_t n, int32_t* __restrict__ v, int32_t* __restrict__ total) {
    __shared__ int64_t wave_total[SF_SCAN_THREADS / 64];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    int64_t carry = 0;
    for (int64_t base = 0; base < n; base += SF_SCAN_THREADS) {
        const int64_t b = base + t;
        const int64_t len = b < n ? v[b] : 0;
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
        for (int i = 0; i < SF_SCAN_THREADS / 64; ++i) { const int64_t x = wave_total[i]; if (i < w) before += x; tile += x; }
        if (b < n) v[b] = (int32_t)(carry + before + incl - len);
        carry += tile;
        __syncthreads();                                           // (wave_total is rewritten by the next tile)
    }
    if (t == 0) *total = (int32_t)carry;
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

// block = 256 >> shift rows x (1 << shift) columns (the power of two >= d4), as tw_gather_kernel
__global__ __launch_bounds__(256) void sf_gather_users_kernel(int n_query, const int64_t* __restrict__ query_users, const float* __restrict__ Eu, int64_t ldu,
                                                              int d, int d4, int shift, float* __restrict__ Ug, int64_t* __restrict__ ident,
                                                              const int32_t* __restrict__ n_kept_dev, int32_t n_kept, uint32_t* __restrict__ err) {
    const int k = threadIdx.x & ((1 << shift) - 1);
    const int64_t q = (int64_t)blockIdx.x * (256 >> shift) + (threadIdx.x >> shift);
    if (blockIdx.x == 0 && threadIdx.x == 0) *err = *n_kept_dev != n_kept ? 1u : 0u;
    if (q >= n_query || k >= d4) return;
    Ug[q * d4 + k] = k < d ? Eu[query_users[q] * ldu + k] : 0.0f;
    if (k == 0) ident[q] = q;
}

__global__ __launch_bounds__(256) void sf_gather_items_kernel(int32_t n_kept, const int32_t* __restrict__ old_id, const int32_t* __restrict__ n_kept_dev,
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

__device__ __forceinline__ bool sf_kept(const int32_t* __restrict__ new_id, int64_t n_items, int32_t c) { return c >= 0 && c < n_items && new_id[c] >= 0; }

__global__ __launch_bounds__(256) void sf_count_kernel(int n_query, const int64_t* __restrict__ query_users, const int32_t* __restrict__ train_rowptr,
                                                       const int32_t* __restrict__ train_colidx, const int32_t* __restrict__ new_id, int64_t n_items,
                                                       int32_t* __restrict__ cnt) {
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= n_query) return;                                      // (wave-uniform; the kernel has no block barrier)
    const int64_t u = query_users[q];
    const int32_t r0 = train_rowptr[u], r1 = train_rowptr[u + 1];
    int n = 0;
    for (int32_t base = r0; base < r1; base += 64) {
        const int32_t e = base + lane;
        n += __popcll(__ballot(e < r1 && sf_kept(new_id, n_items, train_colidx[e < r1 ? e : r0])));
    }
    if (lane == 0) cnt[q] = n;
}

// rowptr[0 .. n_query] = exclusive scan of cnt, as tw_rowptr_kernel; a total beyond cap or a set error word: zeros, and the word stays set
__global__ __launch_bounds__(SF_SCAN_THREADS) void sf_rowptr_kernel(int n_query, const int32_t* __restrict__ cnt, int64_t cap, int32_t* __restrict__ rowptr,
                                                                    uint32_t* __restrict__ err) {
    __shared__ int64_t wave_total[SF_SCAN_THREADS / 64];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const uint32_t was_bad = *err;                                 // (read by every thread before the barriers below; written once, after them)
    int64_t carry = 0;
    for (int64_t base = 0; base < n_query; base += SF_SCAN_THREADS) {
        const int64_t q = base + t;
        const int64_t len = q < n_query ? cnt[q] : 0;
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
        for (int i = 0; i < SF_SCAN_THREADS / 64; ++i) { const int64_t x = wave_total[i]; if (i < w) before += x; tile += x; }
        if (q < n_query) rowptr[q] = (int32_t)(carry + before + incl - len);
        carry += tile;
        __syncthreads();                                           // (wave_total is rewritten by the next tile)
    }
    const bool bad = was_bad != 0u || carry > cap;
    if (bad)
        for (int64_t q = t; q < n_query; q += SF_SCAN_THREADS) rowptr[q] = 0;
    if (t == 0) { rowptr[n_query] = bad ? 0 : (int32_t)carry; *err = bad ? 1u : 0u; }
}

__global__ __launch_bounds__(256) void sf_mask_kernel(int n_query, const int64_t* __restrict__ query_users, const int32_t* __restrict__ train_rowptr,
                                                      const int32_t* __restrict__ train_colidx, const int32_t* __restrict__ new_id, int64_t n_items,
                                                      const int32_t* __restrict__ rowptr, int32_t* __restrict__ colidx, int64_t cap,
                                                      const uint32_t* __restrict__ err) {
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= n_query || *err != 0u) return;                        // (wave-uniform; the kernel has no block barrier)
    const int64_t u = query_users[q];
    const int32_t r0 = train_rowptr[u], r1 = train_rowptr[u + 1];
    int64_t pos = rowptr[q];
    for (int32_t base = r0; base < r1; base += 64) {
        const int32_t e = base + lane;
        const int32_t c = e < r1 ? train_colidx[e] : -1;
        const bool keep = sf_kept(new_id, n_items, c);
        const uint64_t m = __ballot(keep);
        const int64_t at = pos + lanes_below(m, lane);
        if (keep && at < cap) colidx[at] = new_id[c];
        pos += __popcll(m);
    }
}

__global__ __launch_bounds__(256) void sf_map_back_kernel(int64_t n, int32_t n_kept, const int32_t* __restrict__ old_id, int32_t* __restrict__ idx,
                                                          float* __restrict__ score, const uint32_t* __restrict__ err) {
    const bool bad = *err != 0u;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        const int32_t id = idx[e];
        if (bad || id < 0 || id >= n_kept) { idx[e] = -1; score[e] = -INFINITY; }
        else idx[e] = old_id[id];
    }
}

// every list empty (no eligible item: the sweeps refuse an empty table)
__global__ __launch_bounds__(256) void sf_fill_empty_kernel(int64_t n, int32_t* __restrict__ idx, float* __restrict__ score) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) { idx[e] = -1; score[e] = -INFINITY; }
}

// byte offsets, behind the wide call's workspace, of: item rows, user rows, query list, error word, counts, row pointers, mask columns; returns
// their total
static int64_t sf_parts(int32_t n_query, int32_t n_kept, int32_t d, int64_t train_nnz, int64_t* off) {
    const int64_t n = n_query, d4 = align_up(d, 4);
    off[0] = 0;
    off[1] = off[0] + align_up(4 * (int64_t)n_kept * d4, 256);
    off[2] = off[1] + align_up(4 * n * d4, 256);
    off[3] = off[2] + align_up(8 * n, 256);
    off[4] = off[3] + 256;
    off[5] = off[4] + align_up(4 * n, 256);
    off[6] = off[5] + align_up(4 * (n + 1), 256);
    return off[6] + align_up(4 * train_nnz, 256) + 256;           // (+ 256: the columns' base lies inside the workspace at train_nnz = 0 too)
}

static bool sf_sizes_ok(int32_t n_query, int64_t n_items, int32_t n_kept, int32_t d, int32_t K, int64_t train_nnz) {
    return n_query >= 0 && n_items > 0 && n_items < (1ll << 31) && n_kept >= 0 && n_kept <= n_items && d > 0 && d <= 128 && K > 0 &&
           K <= LLMREC_TOPK_WIDE_MAX && train_nnz >= 0 && train_nnz < (1ll << 31);
}

static int sf_shift(int d4) {
    int shift = 2;
    while ((1 << shift) < d4) ++shift;
    return shift;
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
    if_scan_kernel<<<1, SF_SCAN_THREADS, 0, stream>>>(n_blocks, block_cnt, n_kept_dev);
    LLMREC_LAUNCH_CHECK();
    if (n_blocks > 0) {
        if_write_kernel<<<(unsigned)n_blocks, IF_THREADS, 0, stream>>>(n_items, allow, block_cnt, new_id, old_id);
        LLMREC_LAUNCH_CHECK();
    }
    return LLMREC_OK;
}

int64_t llmrec_score_topk_filtered_workspace_bytes(int32_t n_query, int64_t n_items, int32_t n_kept, int32_t d, int32_t K, int64_t train_nnz) {
    if (!sf_sizes_ok(n_query, n_items, n_kept, d, K, train_nnz)) return -1;
    if (n_kept == 0) return 0;
    const int64_t wide = llmrec_score_topk_wide_workspace_bytes(n_query, n_kept, d, K, train_nnz);
    if (wide < 0) return -1;
    int64_t off[7];
    return align_up(wide, 256) + sf_parts(n_query, n_kept, d, train_nnz, off);
}

int64_t llmrec_score_topk_filtered_mask_offset(int32_t n_query, int64_t n_items, int32_t n_kept, int32_t d, int32_t K, int64_t train_nnz) {
    if (!sf_sizes_ok(n_query, n_items, n_kept, d, K, train_nnz) || n_kept == 0) return -1;
    const int64_t wide = llmrec_score_topk_wide_workspace_bytes(n_query, n_kept, d, K, train_nnz);
    if (wide < 0) return -1;
    int64_t off[7];
    sf_parts(n_query, n_kept, d, train_nnz, off);
    return align_up(wide, 256) + off[5];
}

int llmrec_score_topk_filtered_f32(int32_t n_query, const int64_t* query_users,
                                   const float* Eu, int64_t ldu, const float* Ei, int64_t ldi,
                                   int64_t n_items, int32_t d,
                                   const int32_t* train_rowptr, const int32_t* train_colidx,
                                   int32_t K, int32_t* out_idx, float* out_score,
                                   void* workspace, int64_t workspace_bytes, int32_t mode, int64_t train_nnz,
                                   const int32_t* new_id, const int32_t* old_id, const int32_t* n_kept_dev, int32_t n_kept,
                                   llmrec_stream_t stream_) {
    LLMREC_CHECK_ARG(n_query >= 0 && n_items > 0 && n_items < (1ll << 31) && d > 0 && K > 0 && K <= LLMREC_TOPK_WIDE_MAX,
                     "score_topk_filtered: bad sizes (K <= %d, n_items < 2^31)", LLMREC_TOPK_WIDE_MAX);
    LLMREC_CHECK_ARG(n_kept >= 0 && n_kept <= n_items, "score_topk_filtered: n_kept = %d outside [0, n_items]", n_kept);
    LLMREC_CHECK_ARG(mode == LLMREC_TOPK_MODE_EXACT_SWEEP || mode == LLMREC_TOPK_MODE_PREFILTER, "score_topk_filtered: unknown mode %d", mode);
    if (n_query == 0) return LLMREC_OK;
    LLMREC_CHECK_ARG(query_users && Eu && Ei && out_idx && out_score && ldu >= d && ldi >= d, "score_topk_filtered: null pointer or ld < d");
    LLMREC_CHECK_ARG(new_id && old_id && n_kept_dev, "score_topk_filtered: the filter's maps are missing");
    LLMREC_CHECK_ARG((train_rowptr == nullptr) == (train_colidx == nullptr), "score_topk_filtered: train CSR incomplete");
    LLMREC_CHECK_EVAL_WIDTH(d);
    if (!train_rowptr) train_nnz = 0;
    LLMREC_CHECK_ARG(train_nnz >= 0 && train_nnz < (1ll << 31), "score_topk_filtered: train_nnz outside [0, 2^31)");
    hipStream_t stream = (hipStream_t)stream_;
    const int64_t n_out = (int64_t)n_query * K;
    if (n_kept == 0) {                                             // no eligible item: every list is empty, no sweep is launched
        sf_fill_empty_kernel<<<grid_for(n_out, 256), 256, 0, stream>>>(n_out, out_idx, out_score);
        LLMREC_LAUNCH_CHECK();
        return LLMREC_OK;
    }
    const int64_t wide = llmrec_score_topk_wide_workspace_bytes(n_query, n_kept, d, K, train_nnz);
    LLMREC_CHECK_ARG(wide >= 0, "score_topk_filtered: train_nnz + n_query * K must lie in [0, 2^31)");
    int64_t off[7];
    const int64_t need = align_up(wide, 256) + sf_parts(n_query, n_kept, d, train_nnz, off);
    LLMREC_CHECK_ARG(workspace && (uintptr_t)workspace % 16 == 0, "score_topk_filtered: needs the workspace (16-byte aligned)");
    if (workspace_bytes < need) {
        set_error("score_topk_filtered: workspace %lld < %lld", (long long)workspace_bytes, (long long)need);
        return LLMREC_EWORKSPACE;
    }
    char* x = (char*)workspace + align_up(wide, 256);
    float* Ig = (float*)(x + off[0]);
    float* Ug = (float*)(x + off[1]);
    int64_t* ident = (int64_t*)(x + off[2]);
    uint32_t* err = (uint32_t*)(x + off[3]);
    int32_t* cnt = (int32_t*)(x + off[4]);
    int32_t* rowptr = (int32_t*)(x + off[5]);
    int32_t* colidx = (int32_t*)(x + off[6]);
    const int d4 = (int)align_up(d, 4), shift = sf_shift(d4);
    const int rows_per_block = 256 >> shift, wave_grid = (int)ceil_div(n_query, 4);

    sf_gather_users_kernel<<<(unsigned)ceil_div(n_query, rows_per_block), 256, 0, stream>>>(n_query, query_users, Eu, ldu, d, d4, shift, Ug, ident,
                                                                                             n_kept_dev, n_kept, err);
    LLMREC_LAUNCH_CHECK();
    sf_gather_items_kernel<<<(unsigned)ceil_div(n_kept, rows_per_block), 256, 0, stream>>>(n_kept, old_id, n_kept_dev, Ei, ldi, n_items, d, d4, shift, Ig);
    LLMREC_LAUNCH_CHECK();
    if (train_rowptr) {
        sf_count_kernel<<<wave_grid, 256, 0, stream>>>(n_query, query_users, train_rowptr, train_colidx, new_id, n_items, cnt);
        LLMREC_LAUNCH_CHECK();
        sf_rowptr_kernel<<<1, SF_SCAN_THREADS, 0, stream>>>(n_query, cnt, train_nnz, rowptr, err);
        LLMREC_LAUNCH_CHECK();
        sf_mask_kernel<<<wave_grid, 256, 0, stream>>>(n_query, query_users, train_rowptr, train_colidx, new_id, n_items, rowptr, colidx, train_nnz, err);
        LLMREC_LAUNCH_CHECK();
    }
    const int rc = llmrec_score_topk_wide_f32(n_query, ident, Ug, d4, Ig, d4, n_kept, d, train_rowptr ? rowptr : nullptr, train_rowptr ? colidx : nullptr,
                                              K, out_idx, out_score, workspace, wide, mode, train_nnz, stream_);
    if (rc != LLMREC_OK) return rc;
    sf_map_back_kernel<<<grid_for(n_out, 256), 256, 0, stream>>>(n_out, n_kept, old_id, out_idx, out_score, err);
    LLMREC_LAUNCH_CHECK();
    return LLMREC_OK;
}

}  // extern "C"
