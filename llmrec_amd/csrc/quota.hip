// quota.hip - serving: per-group quotas in the lists of candidates.hip ("at most m items of any one brand, seller, series in a user's list").
//
// llmrec_score_topk_candidates_capped_f32 is llmrec_score_topk_candidates_f32 up to the sorted (key, id) pairs - cd_sorted_pairs of
// candidates.hip, the same launches and the same buffers: each query's survivors stand in (score desc, item id asc) order. In place of
// cd_write_kernel:
//   qt_write_kernel    one wave per query: the query's range in the sorted keys (cd_query_range), walked in chunks of 64 entries. Lane l of a
//                      chunk holds entry l with group g (item_group[id]; outside [0, n_groups): no group). Its rank within its group =
//                      base[g], the survivors of g in the chunks before, + the earlier lanes of the chunk with the same g (64 broadcasts);
//                      it is kept iff it has no group or rank < cap(g). A ballot and a prefix popcount give the output slot, a lane writes
//                      if its slot is below K, and the wave stops when K items are taken or the range ends: the walk costs the prefix it
//                      needs. -1 / -inf behind the last item - and everywhere under the error word.
//   base[g]            a per-wave open-addressing table in LDS (keys + counts, 2^s >= 2 K slots, linear probing), keyed by group id. Only a
//                      group LEADER - the first lane of its group in the chunk - touches the table for writing, and only if the leader is
//                      kept: base[g] + the chunk's entries of g. A group that is not in the table has base 0; a group whose leader is not
//                      kept has reached its cap (it is in the table, with a count >= cap, which is all a later chunk asks) or has cap 0.
//                      So the table holds at most one slot per kept item, and the last chunk (K reached) inserts nothing: fewer than K
//                      slots are ever in use. Slots are claimed by integer LDS compare-and-swap among the distinct leaders of one chunk;
//                      which slot a group gets depends on the order, the count read back for a group does not. No global atomics, no
//                      float atomics, no scratch.
// LDS: 8 bytes x slots per wave, sized from K at launch; 4 waves per block while that stays within 32 KiB, else 2 (K = 1024: 2 x 16 KiB).
#include "candidates.h"

namespace llmrec {

constexpr int32_t QT_EMPTY = -1;                                   // (a table key is a group id >= 0)

__device__ __forceinline__ uint32_t qt_hash(int32_t g, int shift) { return ((uint32_t)g * 2654435761u) >> shift; }

// lds: [waves][slots] keys, then [waves][slots] counts; slots = 1 << (32 - shift) >= 64
__global__ __launch_bounds__(256) void qt_write_kernel(int n_query, int K, int waves, int shift, const uint64_t* __restrict__ keys,
                                                       const int32_t* __restrict__ ids, int64_t n_keys, const int32_t* __restrict__ item_group,
                                                       int32_t n_groups, const int32_t* __restrict__ group_cap, int32_t cap,
                                                       int32_t* __restrict__ out_idx, float* __restrict__ out_score, const uint32_t* __restrict__ err) {
    extern __shared__ int32_t qt_lds[];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t q = (int64_t)blockIdx.x * waves + w;
    if (w >= waves || q >= n_query) return;                        // (wave-uniform; no block barrier below)
    const int slots = 1 << (32 - shift);
    int32_t* tkey = qt_lds + w * slots;
    int32_t* tcnt = qt_lds + (waves + w) * slots;
    int64_t lo, hi;
    cd_query_range(keys, n_keys, q, lane, err, lo, hi);
    for (int s = lane; s < slots; s += 64) tkey[s] = QT_EMPTY;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();

    int taken = 0;                                                 // (wave-uniform)
    for (int64_t at = lo; at < hi && taken < K; at += 64) {
        const bool valid = at + lane < hi;
        const int32_t id = valid ? ids[at + lane] : 0;
        const int32_t g = valid ? item_group[id] : -1;             // (a pair of the range carries an item id in [0, n_items))
        const bool grouped = g >= 0 && g < n_groups;
        const int32_t room = grouped ? (group_cap ? group_cap[g] : cap) : 0;
        const int32_t mine = grouped ? g : -1 - lane;              // (a lane without a group matches no other lane)
        int before = 0, total = 0;                                 // the chunk's entries of my group: in earlier lanes, in all
#pragma unroll 8
        for (int l = 0; l < 64; ++l) {                             // (l is wave-uniform: one scalar broadcast per step)
            const bool same = __builtin_amdgcn_readlane(mine, l) == mine;
            before += (same && l < lane) ? 1 : 0;
            total += same ? 1 : 0;
        }
        int32_t base = 0;
        uint32_t h = 0;
        if (grouped && room > 0) {                                 // (cap 0: never kept, never looked up)
            h = qt_hash(g, shift);
            int32_t k;
            while ((k = tkey[h]) != g && k != QT_EMPTY) h = (h + 1) & (slots - 1);
            if (k == g) base = tcnt[h];
        }
        const bool keep = valid && (!grouped || base + before < room);
        const uint64_t kept = __ballot(keep);
        const int slot = taken + lanes_below(kept, lane);
        if (keep && slot < K) {
            out_idx[q * K + slot] = id;
            out_score[q * K + slot] = cd_unordered(~(uint32_t)keys[at + lane]);
        }
        taken += __popcll(kept);
        if (taken >= K) break;                                     // (the last chunk inserts nothing)
        if (keep && grouped && before == 0) {                      // a kept leader: its group's count moves on by the chunk's entries
            while (true) {
                const int32_t old = atomicCAS(&tkey[h], QT_EMPTY, g);
                if (old == QT_EMPTY || old == g) break;
                h = (h + 1) & (slots - 1);
            }
            tcnt[h] = base + total;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    for (int j = (taken < K ? taken : K) + lane; j < K; j += 64) {
        out_idx[q * K + j] = -1;
        out_score[q * K + j] = -INFINITY;
    }
}

// slots per wave: the power of two >= 2 K, at least 64
static int qt_shift(int32_t K) {
    int bits = 6;
    while ((1 << bits) < 2 * K) ++bits;
    return 32 - bits;
}

}  // namespace llmrec

using namespace llmrec;

extern "C" {

int llmrec_score_topk_candidates_capped_f32(int32_t n_query, const int64_t* query_users,
                                            const float* Eu, int64_t ldu, const float* Ei, int64_t ldi, int64_t n_items, int32_t d,
                                            const int32_t* train_rowptr, const int32_t* train_colidx,
                                            int32_t K, int32_t* out_idx, float* out_score, void* workspace, int64_t workspace_bytes,
                                            const int32_t* cand_rowptr, const int32_t* cand_colidx, int64_t cand_nnz,
                                            const int32_t* excl_rowptr, const int32_t* excl_colidx, int64_t excl_nnz,
                                            const int32_t* new_id, const int32_t* item_group, int32_t n_groups, const int32_t* group_cap, int32_t cap,
                                            llmrec_stream_t stream_) {
    const char* name = "score_topk_candidates_capped";
    const CandCall c = {n_query, query_users, Eu, ldu, Ei, ldi, n_items, d, train_rowptr, train_colidx, K, out_idx, out_score, workspace, workspace_bytes,
                        cand_rowptr, cand_colidx, cand_nnz, excl_rowptr, excl_colidx, excl_nnz, new_id};
    int rc = cd_check(name, c);
    if (rc != LLMREC_OK) return rc;
    LLMREC_CHECK_ARG(K <= LLMREC_TOPK_WIDE_MAX, "%s: K = %d exceeds LLMREC_TOPK_WIDE_MAX = %d (K sizes the group table)", name, K, LLMREC_TOPK_WIDE_MAX);
    LLMREC_CHECK_ARG(item_group, "%s: item_group is missing", name);
    LLMREC_CHECK_ARG(n_groups >= 1, "%s: n_groups = %d, at least 1 expected", name, n_groups);
    LLMREC_CHECK_ARG(group_cap || cap >= 1, "%s: cap = %d without group_cap, at least 1 expected", name, cap);
    if (n_query == 0) return LLMREC_OK;
    hipStream_t stream = (hipStream_t)stream_;
    const int shift = qt_shift(K);
    const int64_t per_wave = 8ll << (32 - shift);                  // keys + counts
    const int waves = 4 * per_wave <= (32 << 10) ? 4 : 2;          // (K <= 1024: per_wave <= 16 KiB)
    const unsigned grid = (unsigned)ceil_div(n_query, waves);
    const size_t lds = (size_t)(waves * per_wave);
    CandSorted s = {nullptr, nullptr, nullptr};                    // no candidate entry: every list is empty, one launch
    if (cand_nnz > 0 && (rc = cd_sorted_pairs(name, c, stream, &s)) != LLMREC_OK) return rc;
    qt_write_kernel<<<grid, 64 * waves, lds, stream>>>(n_query, K, waves, shift, s.keys, s.ids, cand_nnz > 0 ? cand_nnz : 0, item_group, n_groups, group_cap, cap,
                                                out_idx, out_score, s.err);
    LLMREC_LAUNCH_CHECK();
    return LLMREC_OK;
}

}  // extern "C"
