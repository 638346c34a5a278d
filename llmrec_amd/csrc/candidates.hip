// candidates.hip - serving: exact top-K among PER-QUERY candidate lists ("here are this request's candidates; rank them for this user"). The
// sweeps of topk.hip are not involved: only the listed pairs are scored, and the selection is two radix sorts.
//
// llmrec_score_topk_candidates_f32, on the caller's one stream:
//   cd_open_kernel     the error word = 0 (the two keys kernels only ever set it)
//   cd_keys_kernel     entry e of candidate row q -> the 64-bit key  q << 32 | ORIGINAL id  (q by binary search in cand_rowptr, as
//                      ex_keys_kernel); an entry < 0, >= n_items or ineligible under the filter -> n_query << 32, behind every row. The same
//                      launch checks cand_rowptr: 0 at the front, cand_nnz at the back, non-decreasing - else the error word
//   (vendor radix sort) the keys over bits [0, 32 + bits(n_query)): rows in order, each ascending by id, repeats adjacent
//   exclude_sorted_keys of exclude.hip with the identity numbering (with an exclusion CSR): the sorted keys  q << 32 | id  of the exclusion rows
//   cd_score_kernel    sorted key e is dropped if it repeats key e - 1, is the dropped key, has its id in the train row of query_users[q] or
//                      has  q << 32 | id  among the exclusion keys (binary searches). Otherwise its score is the k-ordered fp32 fma chain of
//                      tk_finalize_user / auc_chain of topk.hip (restated below: the bits of llmrec_scores_f32), and the pair
//                      (q << 32 | ~m(score), id) goes out, m the order-preserving map of float bits to uint32. A dropped entry: n_query << 32
//   (vendor radix sort) the (key, id) pairs over the same bits. Ascending keys = queries in order, scores descending; the sort is stable and
//                      its input ascends by id inside a query, so equal scores stay in id order (the chain starts at +0 and never gives
//                      -0.0: equal floats are equal keys)
//   cd_write_kernel    one wave per query: the lower bounds of q << 32 and (q + 1) << 32 in the sorted keys; the first min(K, count) ids and
//                      the scores decoded from the keys, -1 / -inf behind them - and everywhere under the error word
// cand_nnz == 0 is one launch of cd_write_kernel (every list empty), n_query == 0 none. Sizes and launch counts come from host arguments
// alone; no allocation, no host read, no atomics, every cross-block hand-over a kernel boundary: capturable and deterministic.
// Everything up to the second sort is cd_sorted_pairs (declared in candidates.h), which the capped entry of quota.hip calls too: that entry
// differs in its last launch alone.
#include "candidates.h"
#include <hipcub/hipcub.hpp>
#include <stdlib.h>

namespace llmrec {

__global__ void cd_open_kernel(uint32_t* __restrict__ err) {
    if (threadIdx.x == 0) *err = 0u;
}

// threads [0, n_query]: the checks of cand_rowptr; threads [0, cand_nnz): the keys. A broken cand_rowptr still gives every entry a row in
// [0, n_query), and the error word empties the call.
__global__ __launch_bounds__(256) void cd_keys_kernel(int n_query, const int32_t* __restrict__ cand_rowptr, const int32_t* __restrict__ cand_colidx,
                                                      int64_t cand_nnz, const int32_t* __restrict__ new_id, int64_t n_items,
                                                      uint64_t* __restrict__ keys, uint32_t* __restrict__ err) {
    const int64_t work = cand_nnz > n_query + 1 ? cand_nnz : n_query + 1;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < work; e += (int64_t)gridDim.x * 256) {
        if (e <= n_query) {
            const int32_t here = cand_rowptr[e];
            const bool bad = e == n_query ? here != cand_nnz : (here > cand_rowptr[e + 1] || (e == 0 && here != 0));
            if (bad) *err = 1u;
        }
        if (e < cand_nnz) {
            int lo = 0, hi = n_query - 1;                          // the last row q with cand_rowptr[q] <= e
            while (lo < hi) {
                const int mid = lo + ((hi - lo + 1) >> 1);
                if (cand_rowptr[mid] <= e) lo = mid; else hi = mid - 1;
            }
            const int32_t id = cand_colidx[e];
            keys[e] = swept_id(new_id, n_items, id) >= 0 ? ((uint64_t)lo << 32) | (uint32_t)id : (uint64_t)n_query << 32;
        }
    }
}

// columns [16 c, 16 c + 16) of a user row and an item row (zeros past d: fmaf(0, 0, acc) == acc, since acc is never -0.0)
__device__ __forceinline__ void cd_load_chunk(const float* ur, const float* ir, int c, int d, bool vec, float4 (&uv)[4], float4 (&iv)[4]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) { uv[q] = load4_guard(ur, 16 * c + 4 * q, d, vec); iv[q] = load4_guard(ir, 16 * c + 4 * q, d, vec); }
}
// 16 steps of the chain of v_mfma_f32_16x16x4_f32: s, then q; k = 16 c + 4 q + s
__device__ __forceinline__ float cd_chain_chunk(float acc, const float4 (&uv)[4], const float4 (&iv)[4]) {
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc = __builtin_fmaf(comp(uv[q], s), comp(iv[q], s), acc);
    return acc;
}

struct CandArgs {
    int n_query;
    const int64_t* query_users;
    const float* Eu; int64_t ldu;
    const float* Ei; int64_t ldi;
    int d; int vec_ok;
    const int32_t* train_rowptr; const int32_t* train_colidx;      // (null: nothing removed)
    const uint64_t* excl; int64_t excl_nnz;                        // the sorted exclusion keys (null: none)
    const uint64_t* keys; int64_t cand_nnz;                        // the sorted candidate keys
    uint64_t* out_key; int32_t* out_id;
    const uint32_t* err;
};

// LANES lanes per pair. 4 (the product's): lane j of the group fetches chunks j and j + 4 (64 contiguous bytes each) up front, then the chain
// runs chunk by chunk, acc handed from lane to lane by shuffle - the same order, the same bits. 1 (the tools build's, for comparison): a
// lane walks its pair's rows, chunk after chunk.
template <int LANES>
__global__ __launch_bounds__(256) void cd_score_kernel(CandArgs a) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t e = t / LANES;
    if (e >= a.cand_nnz || *a.err != 0u) return;                   // (LANES divides 64: a group leaves together)
    const uint64_t dropped = (uint64_t)a.n_query << 32;
    const uint64_t key = a.keys[e];
    const uint32_t q = (uint32_t)(key >> 32);
    const int32_t id = (int32_t)(uint32_t)key;
    bool keep = key < dropped && !(e > 0 && a.keys[e - 1] == key); // (key < dropped: q < n_query, and id was an eligible item)
    const int64_t u = keep ? a.query_users[q] : 0;
    if (keep && a.train_rowptr) {
        int32_t lo = a.train_rowptr[u], hi = a.train_rowptr[u + 1];
        const int32_t end = hi;
        while (lo < hi) { const int32_t mid = lo + ((hi - lo) >> 1); if (a.train_colidx[mid] < id) lo = mid + 1; else hi = mid; }
        if (lo < end && a.train_colidx[lo] == id) keep = false;
    }
    if (keep && a.excl) {
        int64_t lo = 0, hi = a.excl_nnz;
        while (lo < hi) { const int64_t mid = lo + ((hi - lo) >> 1); if (a.excl[mid] < key) lo = mid + 1; else hi = mid; }
        if (lo < a.excl_nnz && a.excl[lo] == key) keep = false;
    }
    const float* ur = a.Eu + u * a.ldu;
    const float* ir = a.Ei + (int64_t)(keep ? id : 0) * a.ldi;
    const bool vec = a.vec_ok != 0;
    float acc = 0.f;
    if (LANES == 1) {
        if (keep) {
#pragma unroll 1
            for (int c = 0; 16 * c < a.d; ++c) {
                float4 uv[4], iv[4];
                cd_load_chunk(ur, ir, c, a.d, vec, uv, iv);
                acc = cd_chain_chunk(acc, uv, iv);
            }
        }
    } else {
        const int lane = threadIdx.x & 63, sub = lane & (LANES - 1), base = lane & ~(LANES - 1);
        const bool two = a.d > 16 * LANES;                         // (wave-uniform)
        float4 u0[4], i0[4], u1[4], i1[4];
        const int dk = keep ? a.d : 0;                             // (a dropped pair loads nothing: zeros)
        cd_load_chunk(ur, ir, sub, dk, vec, u0, i0);
        if (two) cd_load_chunk(ur, ir, sub + LANES, dk, vec, u1, i1);
#pragma unroll
        for (int c = 0; c < LANES; ++c) {
            const float prev = c == 0 ? 0.f : __shfl(acc, base + c - 1, 64);
            const float r = cd_chain_chunk(prev, u0, i0);
            if (sub == c) acc = r;
        }
        if (two) {
#pragma unroll
            for (int c = 0; c < LANES; ++c) {
                const float prev = __shfl(acc, base + ((c + LANES - 1) & (LANES - 1)), 64);
                const float r = cd_chain_chunk(prev, u1, i1);
                if (sub == c) acc = r;
            }
        }
        if (sub != LANES - 1) return;                              // (the last lane of the group holds the whole chain)
    }
    a.out_key[e] = keep ? ((uint64_t)q << 32) | (uint32_t)~cd_ordered(acc) : dropped;
    a.out_id[e] = id;
}

// wave q: the range of query q in the sorted keys (cd_query_range of candidates.h), its first min(K, count) pairs
__global__ __launch_bounds__(256) void cd_write_kernel(int n_query, int K, const uint64_t* __restrict__ keys, const int32_t* __restrict__ ids, int64_t n_keys,
                                                       int32_t* __restrict__ out_idx, float* __restrict__ out_score, const uint32_t* __restrict__ err) {
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= n_query) return;                                      // (wave-uniform)
    int64_t lo, hi;
    cd_query_range(keys, n_keys, q, lane, err, lo, hi);                // (err == nullptr: no candidate entry at all)
    const int64_t count = hi - lo;
    for (int j = lane; j < K; j += 64) {
        const bool in = j < count;
        out_idx[q * K + j] = in ? ids[lo + j] : -1;
        out_score[q * K + j] = in ? cd_unordered(~(uint32_t)keys[lo + j]) : -INFINITY;
    }
}

// the key bits the sorts must order: 32 of the low word + those of n_query (the key of a dropped entry); ex_end_bit of exclude.hip
static int cd_end_bit(int32_t n_query) {
    int bits = 1;
    while (bits < 31 && ((int64_t)1 << bits) <= n_query) ++bits;
    return 32 + bits;
}

enum { CD_ERR, CD_KEYS_A, CD_KEYS_B, CD_IDS_A, CD_IDS_B, CD_SORT, CD_EX_A, CD_EX_B, CD_EX_SORT, CD_PARTS };

// byte offsets of: error word, candidate keys x 2, ids x 2, the candidate sorts' temporary storage, exclusion keys x 2, the exclusion sort's
// temporary storage; returns their total
static int64_t cd_parts(int64_t cand_nnz, int64_t excl_nnz, int64_t* off) {
    off[CD_ERR] = 0;
    off[CD_KEYS_A] = 256;
    off[CD_KEYS_B] = off[CD_KEYS_A] + align_up(8 * cand_nnz, 256);
    off[CD_IDS_A] = off[CD_KEYS_B] + align_up(8 * cand_nnz, 256);
    off[CD_IDS_B] = off[CD_IDS_A] + align_up(4 * cand_nnz, 256);
    off[CD_SORT] = off[CD_IDS_B] + align_up(4 * cand_nnz, 256);
    off[CD_EX_A] = off[CD_SORT] + exclude_sort_reserve(cand_nnz);
    off[CD_EX_B] = off[CD_EX_A] + align_up(8 * excl_nnz, 256);
    off[CD_EX_SORT] = off[CD_EX_B] + align_up(8 * excl_nnz, 256);
    return off[CD_EX_SORT] + exclude_sort_reserve(excl_nnz);
}

static bool cd_sizes_ok(int32_t n_query, int32_t K, int64_t cand_nnz, int64_t excl_nnz) {
    return n_query >= 0 && K >= 1 && (int64_t)n_query * K < (1ll << 31) && cand_nnz >= 0 && cand_nnz < (1ll << 31) && excl_nnz >= 0 &&
           excl_nnz < (1ll << 31);
}

// lanes per pair of the score kernel: 4 (measured against 1: profiles/experiments/serve_candidates.md). Only the tools build holds the
// rejected mapping, and reads the choice from the environment per call, for tools/candidates_probe.py --lanes
#ifdef LLMREC_TOOLS_BUILD
static int cd_lanes() {
    const char* s = getenv("LLMREC_CAND_LANES");
    return s && atoi(s) == 1 ? 1 : 4;
}
#endif

int cd_check(const char* name, const CandCall& c) {
    LLMREC_CHECK_ARG(c.n_query >= 0 && c.n_items > 0 && c.n_items < (1ll << 31) && c.d >= 1 && c.d <= 128 && c.K >= 1,
                     "%s: bad sizes (1 <= d <= 128, K >= 1, 0 < n_items < 2^31)", name);
    LLMREC_CHECK_ARG((int64_t)c.n_query * c.K < (1ll << 31), "%s: n_query * K must lie below 2^31", name);
    LLMREC_CHECK_ARG(c.cand_nnz >= 0 && c.cand_nnz < (1ll << 31), "%s: cand_nnz outside [0, 2^31)", name);
    LLMREC_CHECK_ARG(c.excl_nnz >= 0 && c.excl_nnz < (1ll << 31), "%s: excl_nnz outside [0, 2^31)", name);
    if (c.n_query == 0) return LLMREC_OK;
    LLMREC_CHECK_ARG(c.query_users && c.Eu && c.Ei && c.out_idx && c.out_score && c.ldu >= c.d && c.ldi >= c.d, "%s: null pointer or ld < d", name);
    LLMREC_CHECK_ARG((c.train_rowptr == nullptr) == (c.train_colidx == nullptr), "%s: train CSR incomplete", name);
    LLMREC_CHECK_ARG(c.cand_rowptr, "%s: cand_rowptr is missing", name);
    LLMREC_CHECK_ARG(c.cand_colidx || c.cand_nnz == 0, "%s: cand_nnz > 0 without cand_colidx", name);
    LLMREC_CHECK_ARG(c.excl_rowptr || c.excl_nnz == 0, "%s: excl_nnz > 0 without excl_rowptr", name);
    LLMREC_CHECK_ARG(c.excl_colidx || c.excl_nnz == 0, "%s: excl_nnz > 0 without excl_colidx", name);
    return LLMREC_OK;
}

int cd_sorted_pairs(const char* name, const CandCall& c, hipStream_t stream, CandSorted* out) {
    const int32_t n_query = c.n_query;
    const int64_t cand_nnz = c.cand_nnz, excl_nnz = c.excl_nnz;
    int64_t off[CD_PARTS];
    const int64_t need = cd_parts(cand_nnz, excl_nnz, off);
    LLMREC_CHECK_ARG(c.workspace && (uintptr_t)c.workspace % 16 == 0, "%s: needs the workspace (16-byte aligned)", name);
    if (c.workspace_bytes < need) {
        set_error("%s: workspace %lld < %lld", name, (long long)c.workspace_bytes, (long long)need);
        return LLMREC_EWORKSPACE;
    }
    char* x = (char*)c.workspace;
    uint32_t* err = (uint32_t*)(x + off[CD_ERR]);
    hipcub::DoubleBuffer<uint64_t> kbuf((uint64_t*)(x + off[CD_KEYS_A]), (uint64_t*)(x + off[CD_KEYS_B]));
    void* temp = x + off[CD_SORT];
    const int n = (int)cand_nnz, end_bit = cd_end_bit(n_query);
    int rc;

    // what the three sorts ask for, before the first launch
    size_t need_keys = 0, need_pairs = 0, need_excl = 0;
    {
        hipcub::DoubleBuffer<uint64_t> k0(nullptr, nullptr);
        hipcub::DoubleBuffer<int32_t> v0(nullptr, nullptr);
        LLMREC_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, need_keys, k0, n, 0, end_bit, stream));
        LLMREC_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, need_pairs, k0, v0, n, 0, end_bit, stream));
        const size_t most = need_keys > need_pairs ? need_keys : need_pairs;
        if (most > (size_t)exclude_sort_reserve(cand_nnz)) {
            set_error("%s: the sort needs %zu B of temporary storage > %lld", name, most, (long long)exclude_sort_reserve(cand_nnz));
            return LLMREC_EWORKSPACE;
        }
    }
    if (c.excl_rowptr && (rc = exclude_sort_need(name, n_query, excl_nnz, &need_excl, stream)) != LLMREC_OK) return rc;

    cd_open_kernel<<<1, 64, 0, stream>>>(err);
    LLMREC_LAUNCH_CHECK();
    const int64_t work = cand_nnz > (int64_t)n_query + 1 ? cand_nnz : (int64_t)n_query + 1;
    cd_keys_kernel<<<grid_for(work, 256), 256, 0, stream>>>(n_query, c.cand_rowptr, c.cand_colidx, cand_nnz, c.new_id, c.n_items, kbuf.Current(), err);
    LLMREC_LAUNCH_CHECK();
    LLMREC_HIP(hipcub::DeviceRadixSort::SortKeys(temp, need_keys, kbuf, n, 0, end_bit, stream));
    const uint64_t* excl = nullptr;
    if (c.excl_rowptr && (rc = exclude_sorted_keys(n_query, c.excl_rowptr, c.excl_colidx, excl_nnz, nullptr, c.n_items, (uint64_t*)(x + off[CD_EX_A]),
                                                   (uint64_t*)(x + off[CD_EX_B]), x + off[CD_EX_SORT], need_excl, err, &excl, stream)) != LLMREC_OK)
        return rc;

    CandArgs a;
    a.n_query = n_query; a.query_users = c.query_users;
    a.Eu = c.Eu; a.ldu = c.ldu; a.Ei = c.Ei; a.ldi = c.ldi; a.d = c.d;
    a.vec_ok = (c.ldu % 4 == 0) && (c.ldi % 4 == 0) && (((uintptr_t)c.Eu | (uintptr_t)c.Ei) % 16 == 0);
    a.train_rowptr = c.train_rowptr; a.train_colidx = c.train_colidx;
    a.excl = excl_nnz > 0 ? excl : nullptr; a.excl_nnz = excl_nnz;
    a.keys = kbuf.Current(); a.cand_nnz = cand_nnz;
    a.out_key = kbuf.Alternate(); a.out_id = (int32_t*)(x + off[CD_IDS_A]);
    a.err = err;
#ifdef LLMREC_TOOLS_BUILD
    if (cd_lanes() == 1) cd_score_kernel<1><<<(unsigned)ceil_div(cand_nnz, 256), 256, 0, stream>>>(a);
    else
#endif
    cd_score_kernel<4><<<(unsigned)ceil_div(4 * cand_nnz, 256), 256, 0, stream>>>(a);
    LLMREC_LAUNCH_CHECK();

    hipcub::DoubleBuffer<uint64_t> sbuf(kbuf.Alternate(), kbuf.Current());
    hipcub::DoubleBuffer<int32_t> vbuf((int32_t*)(x + off[CD_IDS_A]), (int32_t*)(x + off[CD_IDS_B]));
    LLMREC_HIP(hipcub::DeviceRadixSort::SortPairs(temp, need_pairs, sbuf, vbuf, n, 0, end_bit, stream));
    out->keys = sbuf.Current(); out->ids = vbuf.Current(); out->err = err;
    return LLMREC_OK;
}

}  // namespace llmrec

using namespace llmrec;

extern "C" {

int64_t llmrec_score_topk_candidates_workspace_bytes(int32_t n_query, int32_t K, int64_t cand_nnz, int64_t excl_nnz) {
    if (!cd_sizes_ok(n_query, K, cand_nnz, excl_nnz)) return -1;
    if (n_query == 0 || cand_nnz == 0) return 0;
    int64_t off[CD_PARTS];
    return cd_parts(cand_nnz, excl_nnz, off);
}

int llmrec_score_topk_candidates_f32(int32_t n_query, const int64_t* query_users,
                                     const float* Eu, int64_t ldu, const float* Ei, int64_t ldi, int64_t n_items, int32_t d,
                                     const int32_t* train_rowptr, const int32_t* train_colidx,
                                     int32_t K, int32_t* out_idx, float* out_score, void* workspace, int64_t workspace_bytes,
                                     const int32_t* cand_rowptr, const int32_t* cand_colidx, int64_t cand_nnz,
                                     const int32_t* excl_rowptr, const int32_t* excl_colidx, int64_t excl_nnz,
                                     const int32_t* new_id, llmrec_stream_t stream_) {
    const char* name = "score_topk_candidates";
    const CandCall c = {n_query, query_users, Eu, ldu, Ei, ldi, n_items, d, train_rowptr, train_colidx, K, out_idx, out_score, workspace, workspace_bytes,
                        cand_rowptr, cand_colidx, cand_nnz, excl_rowptr, excl_colidx, excl_nnz, new_id};
    int rc = cd_check(name, c);
    if (rc != LLMREC_OK || n_query == 0) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    const unsigned wave_grid = (unsigned)ceil_div(n_query, 4);
    if (cand_nnz == 0) {                                           // no candidate entry: every list is empty
        cd_write_kernel<<<wave_grid, 256, 0, stream>>>(n_query, K, nullptr, nullptr, 0, out_idx, out_score, nullptr);
        LLMREC_LAUNCH_CHECK();
        return LLMREC_OK;
    }
    CandSorted s;
    if ((rc = cd_sorted_pairs(name, c, stream, &s)) != LLMREC_OK) return rc;
    cd_write_kernel<<<wave_grid, 256, 0, stream>>>(n_query, K, s.keys, s.ids, cand_nnz, out_idx, out_score, s.err);
    LLMREC_LAUNCH_CHECK();
    return LLMREC_OK;
}

}  // extern "C"
