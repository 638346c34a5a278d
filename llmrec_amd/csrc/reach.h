// reach.h - the marking half of llmrec_batch_reach_rows as a device function over a VIRTUAL block id, so that it runs as a launch of
// its own (rowops.hip) or as the trailing blocks of the scatter plan's body (guests.h: llmrec_bpr_scatter_plan_reach_mark, and as a guest of a
// grouped SpMM launch).
#pragma once
#include "common.h"

namespace llmrec {

constexpr int REACH_SPLIT = 8;                             // wavefronts per (sample, item): a hub item's adjacency list is walked in 8 interleaved parts

static inline int64_t reach_mark_blocks(int B_cap, int nt = 256) { return ceil_div(3 * (int64_t)B_cap * REACH_SPLIT, nt / 64); }   // nt-thread blocks

// one wavefront per (sample, role, part) - role 0 flags the sample's user, roles 1 / 2 every user in the adjacency list of its
// positive / negative item. vb: the block's index among reach_mark_blocks(B_cap, NT) blocks of NT threads.
template <int NT = 256>
__device__ __forceinline__ void batch_reach_mark_block(int vb, int B_cap, const int32_t* __restrict__ n_valid, const int64_t* __restrict__ users,
                                                       const int64_t* __restrict__ pos, const int64_t* __restrict__ neg, int64_t n_users,
                                                       int64_t n_items, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ colidx,
                                                       uint8_t* __restrict__ flags) {
    const int w = vb * (NT / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    int nv = n_valid ? *n_valid : B_cap;
    nv = nv < B_cap ? nv : B_cap;
    const int part = w % REACH_SPLIT, job = w / REACH_SPLIT;
    const int b = job / 3, role = job - 3 * b;
    if (b >= nv) return;
    if (role == 0) {
        const int64_t u = users[b];
        if (part == 0 && lane == 0 && u >= 0 && u < n_users) flags[u] = 1;
        return;
    }
    const int64_t it = role == 1 ? pos[b] : neg[b];
    if (it < 0 || it >= n_items) return;
    const int32_t s = rowptr[it], e = rowptr[it + 1];
    for (int32_t k = s + part * 64 + lane; k < e; k += 64 * REACH_SPLIT) flags[colidx[k]] = 1;
}

}  // namespace llmrec
