// candidates.h - what candidates.hip (llmrec_score_topk_candidates_f32) and quota.hip (llmrec_score_topk_candidates_capped_f32) share: the
// arguments of a candidate call, its checks, stages (a) to (f) - everything up to the sorted (key, id) pairs - as ONE host function defined
// in candidates.hip, and the device pieces of the last launch: the key's score field and a query's range in the sorted keys. Nothing else
// includes it.
#pragma once
#include "compact.h"

namespace llmrec {

// the order-preserving map of float bits to uint32 (a larger float is a larger word) and back
__device__ __forceinline__ uint32_t cd_ordered(float x) {
    const uint32_t b = __float_as_uint(x);
    return (b & 0x80000000u) ? ~b : b | 0x80000000u;
}
__device__ __forceinline__ float cd_unordered(uint32_t m) { return __uint_as_float((m & 0x80000000u) ? m ^ 0x80000000u : ~m); }

// wave q of a write kernel: lanes 0 and 1 find where the keys of query q begin and end in the sorted keys (the dropped keys lie behind every
// query); every lane returns with the range. Empty under the error word, and with err == nullptr (no candidate entry at all).
__device__ __forceinline__ void cd_query_range(const uint64_t* __restrict__ keys, int64_t n_keys, int64_t q, int lane, const uint32_t* __restrict__ err,
                                               int64_t& lo, int64_t& hi) {
    lo = 0; hi = 0;
    if (err && *err == 0u) {
        const uint64_t head = (uint64_t)(q + (lane & 1)) << 32;
        hi = n_keys;
        while (lo < hi) { const int64_t mid = lo + ((hi - lo) >> 1); if (keys[mid] < head) lo = mid + 1; else hi = mid; }
        hi = __shfl(lo, 1, 64);
        lo = __shfl(lo, 0, 64);
    }
}

// the arguments of llmrec_score_topk_candidates_f32, which the capped entry repeats
struct CandCall {
    int32_t n_query; const int64_t* query_users;
    const float* Eu; int64_t ldu; const float* Ei; int64_t ldi; int64_t n_items; int32_t d;
    const int32_t* train_rowptr; const int32_t* train_colidx;
    int32_t K; int32_t* out_idx; float* out_score; void* workspace; int64_t workspace_bytes;
    const int32_t* cand_rowptr; const int32_t* cand_colidx; int64_t cand_nnz;
    const int32_t* excl_rowptr; const int32_t* excl_colidx; int64_t excl_nnz;
    const int32_t* new_id;
};

// what stages (a) to (f) leave in the workspace: the pairs sorted by (query, score desc, id asc), cand_nnz of them, and the error word
struct CandSorted {
    const uint64_t* keys; const int32_t* ids; const uint32_t* err;
};

// The argument checks of both entries, in `name`'s words: LLMREC_EINVAL, or LLMREC_OK. The pointers are checked only with n_query > 0 (a call
// without queries launches nothing and reads nothing).
int cd_check(const char* name, const CandCall& c);
// Stages (a) to (f) on `stream` for a checked call with n_query > 0 and cand_nnz > 0: the workspace checks, what the sorts ask for, the error
// word, the keys, the first sort, the exclusion keys, the scores, the second sort. The launches and the buffers of the uncapped entry: it IS
// that entry up to its last launch.
int cd_sorted_pairs(const char* name, const CandCall& c, hipStream_t stream, CandSorted* out);

}  // namespace llmrec
