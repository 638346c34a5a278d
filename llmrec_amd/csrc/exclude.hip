// exclude.hip - serving: the exclusion stage of the pipeline of serve.hip - per-QUERY exclusion lists, which arrive unsorted, with repeats and
// with padding, become part of the mask rows the sweeps read. serve.hip calls the three host functions below (declared in common.h) between
// its own launches and owns every buffer; the error word is only ever set to 1 here, by plain stores behind the launch that opened it.
//   ex_keys_kernel          entry e of exclusion row q -> the 64-bit key  q << 32 | id  (q by binary search in excl_rowptr; id in the swept
//                           numbering); an entry < 0, >= n_items or ineligible -> n_query << 32, which sorts behind every row. The same
//                           launch checks excl_rowptr: 0 at the front, excl_nnz at the back, non-decreasing - else the error word
//   (vendor radix sort)     the keys over bits [0, 32 + bits(n_query)), between two buffers of the workspace: rows in order, each ascending
//   ex_merge_kernel         one wave per query, wave-strided: a train entry lands at its index + the number of the query's keys BELOW it, a key
//                           at its index + the number of train entries AT OR BELOW it (binary searches; no LDS, no order carried from one
//                           round to the next): the stable ascending merge, duplicates kept on both sides, train entries first among equals
#include "compact.h"
#include <hipcub/hipcub.hpp>

namespace llmrec {

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
            const int32_t id = swept_id(new_id, n_items, excl_colidx[e]);
            keys[e] = id >= 0 ? ((uint64_t)lo << 32) | (uint32_t)id : (uint64_t)n_query << 32;
        }
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

// the key bits the sort must order: 32 of the id + those of n_query (the key of a dropped entry)
static int ex_end_bit(int32_t n_query) {
    int bits = 1;
    while (bits < 31 && ((int64_t)1 << bits) <= n_query) ++bits;
    return 32 + bits;
}

int exclude_sort_need(const char* name, int32_t n_query, int64_t excl_nnz, size_t* need, hipStream_t stream) {
    *need = 0;
    if (excl_nnz == 0) return LLMREC_OK;
    hipcub::DoubleBuffer<uint64_t> kbuf(nullptr, nullptr);
    LLMREC_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, *need, kbuf, (int)excl_nnz, 0, ex_end_bit(n_query), stream));
    if (*need > (size_t)exclude_sort_reserve(excl_nnz)) {
        set_error("%s: the sort needs %zu B of temporary storage > %lld", name, *need, (long long)exclude_sort_reserve(excl_nnz));
        return LLMREC_EWORKSPACE;
    }
    return LLMREC_OK;
}

int exclude_sorted_keys(int32_t n_query, const int32_t* excl_rowptr, const int32_t* excl_colidx, int64_t excl_nnz, const int32_t* new_id, int64_t n_items,
                        uint64_t* keys_a, uint64_t* keys_b, void* temp, size_t need, uint32_t* err, const uint64_t** sorted, hipStream_t stream) {
    if (excl_rowptr) {
        const int64_t work = excl_nnz > (int64_t)n_query + 1 ? excl_nnz : (int64_t)n_query + 1;
        ex_keys_kernel<<<grid_for(work, 256), 256, 0, stream>>>(n_query, excl_rowptr, excl_colidx, excl_nnz, new_id, n_items, keys_a, err);
        LLMREC_LAUNCH_CHECK();
    }
    hipcub::DoubleBuffer<uint64_t> kbuf(keys_a, keys_b);
    if (excl_nnz > 0) LLMREC_HIP(hipcub::DeviceRadixSort::SortKeys(temp, need, kbuf, (int)excl_nnz, 0, ex_end_bit(n_query), stream));
    *sorted = kbuf.Current();                                      // (which buffer: settled on the host)
    return LLMREC_OK;
}

int exclude_merge_rows(int32_t n_query, const int32_t* trp, const int32_t* tcol, const int32_t* kbeg, const uint64_t* sorted, const int32_t* rp,
                       int32_t* colidx, int64_t cap, const uint32_t* err, hipStream_t stream) {
    ex_merge_kernel<<<(unsigned)ceil_div(n_query, 4), 256, 0, stream>>>(n_query, trp, tcol, kbeg, sorted, rp, colidx, cap, err);
    LLMREC_LAUNCH_CHECK();
    return LLMREC_OK;
}

}  // namespace llmrec
