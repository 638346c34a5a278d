// common.h - shared host/device helpers for the gfx950 kernels (wave = 64 lanes).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include "../../include/llmrec_hip.h"

namespace llmrec {

void set_error(const char* fmt, ...);

#define LLMREC_CHECK_ARG(cond, ...)                                   \
    do {                                                              \
        if (!(cond)) {                                                \
            ::llmrec::set_error(__VA_ARGS__);                         \
            return LLMREC_EINVAL;                                     \
        }                                                             \
    } while (0)

// the evaluation sweeps (scores, top-K, wide rounds) have instances for up to 8 chunks of 16 columns; an entry refuses a wider table
// next to its argument checks, before its first launch
#define LLMREC_CHECK_EVAL_WIDTH(d)                                    \
    do {                                                              \
        if ((d) > 128) {                                              \
            ::llmrec::set_error("score_topk: d = %d > 128", (int)(d)); \
            return LLMREC_EUNSUPPORTED;                               \
        }                                                             \
    } while (0)

#define LLMREC_HIP(call)                                                                   \
    do {                                                                                   \
        hipError_t e__ = (call);                                                           \
        if (e__ != hipSuccess) {                                                           \
            ::llmrec::set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e__), __FILE__, __LINE__); \
            return LLMREC_EHIP;                                                            \
        }                                                                                  \
    } while (0)

// after a kernel launch: catches bad launch configurations without synchronising
#define LLMREC_LAUNCH_CHECK()                                                              \
    do {                                                                                   \
        hipError_t e__ = hipGetLastError();                                                \
        if (e__ != hipSuccess) {                                                           \
            ::llmrec::set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(e__), __FILE__, __LINE__); \
            return LLMREC_EHIP;                                                            \
        }                                                                                  \
    } while (0)

// csrc/topk_wide.hip: the wave-per-user first launch of llmrec_topk_eval_sums for lists of more than 128 columns (partial[block][4 n_ks])
int topk_eval_sums_wide_partials(int32_t n_query, const int64_t* query_users, int32_t K, const int32_t* topk_idx, const int32_t* rowptr,
                                 const int32_t* colidx, int32_t n_ks, const int32_t* ks_host, double* partial, hipStream_t stream);

static inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
static inline int64_t align_up(int64_t a, int64_t b) { return ceil_div(a, b) * b; }

// csrc/exclude.hip: the exclusion stage of the serving pipeline (csrc/serve.hip), on the pipeline's stream. The bytes the pipeline reserves for
// the vendor sort of excl_nnz 64-bit keys (the bound llmrec_scatter_rows_workspace_bytes gives the same sort) ...
static inline int64_t exclude_sort_reserve(int64_t excl_nnz) { return excl_nnz > 0 ? align_up(excl_nnz + (32ll << 20), 256) : 0; }
// ... what the sort asks for, before the call's first launch (more than the reserve: LLMREC_EWORKSPACE in `name`'s words) ...
int exclude_sort_need(const char* name, int32_t n_query, int64_t excl_nnz, size_t* need, hipStream_t stream);
// ... the keys  q << 32 | id  of the exclusion rows and the checks of excl_rowptr (one launch, with an exclusion CSR), then the sort
// (excl_nnz > 0); *sorted = the buffer that holds the rows in order, each ascending ...
int exclude_sorted_keys(int32_t n_query, const int32_t* excl_rowptr, const int32_t* excl_colidx, int64_t excl_nnz, const int32_t* new_id, int64_t n_items,
                        uint64_t* keys_a, uint64_t* keys_b, void* temp, size_t need, uint32_t* err, const uint64_t** sorted, hipStream_t stream);
// ... and mask row q = the stable ascending merge of train row q (trp, tcol) and the query's keys [kbeg[q], kbeg[q + 1]) (one launch)
int exclude_merge_rows(int32_t n_query, const int32_t* trp, const int32_t* tcol, const int32_t* kbeg, const uint64_t* sorted, const int32_t* rp,
                       int32_t* colidx, int64_t cap, const uint32_t* err, hipStream_t stream);

// grid size for a grid-stride kernel: enough blocks to fill 256 CUs x 8, never more than needed
static inline int grid_for(int64_t work_items, int per_block, int max_blocks = 256 * 8) {
    int64_t b = ceil_div(work_items, per_block);
    if (b < 1) b = 1;
    if (b > max_blocks) b = max_blocks;
    return (int)b;
}

#ifdef __HIPCC__
// butterfly sum over the `width` lanes of an aligned lane group (width = power of two <= 64)
template <int WIDTH>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int off = WIDTH / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
template <int WIDTH>
__device__ __forceinline__ float group_max(float v) {
#pragma unroll
    for (int off = WIDTH / 2; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}

// --- primitives that more than one file must spell the same way (each exists once, here) ---
typedef float f32x4 __attribute__((ext_vector_type(4)));      // an MFMA accumulator
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));    // a bf16 MFMA operand

// elements [k, k+4) of a row of length K; zero beyond K
__device__ __forceinline__ float4 load4_guard(const float* row, int k, int K, bool vec_ok) {
    if (vec_ok && k + 3 < K) return *reinterpret_cast<const float4*>(row + k);
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    if (k < K) r.x = row[k];
    if (k + 1 < K) r.y = row[k + 1];
    if (k + 2 < K) r.z = row[k + 2];
    if (k + 3 < K) r.w = row[k + 3];
    return r;
}
__device__ __forceinline__ float comp(const float4& v, int s) { return s == 0 ? v.x : (s == 1 ? v.y : (s == 2 ? v.z : v.w)); }

__device__ __forceinline__ f32x4 mfma_bf16(const uint4& a, const uint4& b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
// high halves of e0 (-> low half of the result) and e1 (-> high half) in one v_perm_b32: no masking needed
__device__ __forceinline__ uint32_t pack_hi16(uint32_t e0, uint32_t e1) { return __builtin_amdgcn_perm(e1, e0, 0x07060302u); }

// fp32 -> bf16, round to nearest even, as the high half of a word (low 16 bits zero): of a FINITE float ...
__device__ __forceinline__ uint32_t rn_bf16_bits_finite(float x) {
    const uint32_t b = __float_as_uint(x);
    return (b + 0x7fffu + ((b >> 16) & 1u)) & 0xffff0000u;
}
// ... and of any float: a NaN stays a quiet NaN
__device__ __forceinline__ uint32_t rn_bf16_bits(float x) {
    if ((__float_as_uint(x) & 0x7fffffffu) > 0x7f800000u) return 0x7fc00000u;
    return rn_bf16_bits_finite(x);
}
#endif

}  // namespace llmrec
