// compact.h - the device pieces of the compaction layers in front of the sweeps, each defined once: topk_wide.hip (the rounds), serve.hip (the
// serving pipeline), exclude.hip (its exclusion stage) and candidates.h (the candidate lists and their quotas: swept_id, lanes_below) include it;
// nothing else does.
#pragma once
#include "common.h"

namespace llmrec {

constexpr int SCAN_THREADS = 1024;                                // the one block of a row-pointer scan: a tile of 1024 elements, 16 waves

// the set bits of a ballot in the lanes below mine
__device__ __forceinline__ int lanes_below(uint64_t mask, int lane) { return __popcll(mask & ((1ull << lane) - 1ull)); }

// the id of item c in the numbering of the table that is swept, or -1: out of range, or ineligible under the filter (new_id == nullptr: no
// filter, the items are numbered as they are)
__device__ __forceinline__ int32_t swept_id(const int32_t* __restrict__ new_id, int64_t n_items, int32_t c) {
    if (c < 0 || c >= n_items) return -1;
    return new_id ? new_id[c] : c;
}

// Exclusive scan over elements [0, n) by ONE block of THREADS threads; every thread must call it (block barriers inside). The block walks the
// elements in tiles of THREADS, thread t on element base + t (neighbouring lanes touch neighbouring entries): inclusive scan inside each wave
// by shuffles, the wave totals through LDS and summed in index order, a running carry from tile to tile - int64 sums in a fixed order.
// len_of(i) is the length of element i, store(i, prefix) receives the sum of the lengths before it; both are called for i < n only, by the
// thread that owns i. Returns the total, in every thread. What a caller reads once for the whole block (an error word) it reads before the
// call and writes after it.
template <int THREADS, class Len, class Store>
__device__ __forceinline__ int64_t block_exclusive_scan(int64_t n, Len len_of, Store store) {
    static_assert(THREADS % 64 == 0, "whole waves");
    __shared__ int64_t wave_total[THREADS / 64];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    int64_t carry = 0;
    for (int64_t base = 0; base < n; base += THREADS) {
        const int64_t i = base + t;
        const int64_t len = i < n ? len_of(i) : 0;
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
        for (int x = 0; x < THREADS / 64; ++x) { const int64_t v = wave_total[x]; if (x < w) before += v; tile += v; }
        if (i < n) store(i, carry + before + incl - len);
        carry += tile;
        __syncthreads();                                           // (wave_total is rewritten by the next tile)
    }
    return carry;
}

// The queried user rows as a compact [n_query][d4] table (zero pad columns; copied values give the same score bits) + the identity query
// list. Block = 256 >> shift queries x (1 << shift) columns (the power of two >= d4): no division per element. first(q) runs in the thread
// that writes ident[q], for what else a caller keeps per query.
template <class First>
__device__ __forceinline__ void gather_user_rows(int n_query, const int64_t* __restrict__ query_users, const float* __restrict__ Eu, int64_t ldu, int d,
                                                 int d4, int shift, float* __restrict__ Ug, int64_t* __restrict__ ident, First first) {
    const int k = threadIdx.x & ((1 << shift) - 1);
    const int64_t q = (int64_t)blockIdx.x * (256 >> shift) + (threadIdx.x >> shift);
    if (q >= n_query || k >= d4) return;
    Ug[q * d4 + k] = k < d ? Eu[query_users[q] * ldu + k] : 0.0f;
    if (k == 0) { ident[q] = q; first(q); }
}

// the shift of gather_user_rows' launch: the power of two >= d4, at least 4 columns
static inline int gather_shift(int d4) {
    int shift = 2;
    while ((1 << shift) < d4) ++shift;
    return shift;
}

}  // namespace llmrec
