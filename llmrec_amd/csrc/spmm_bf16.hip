// spmm_bf16.hip - the SpMM that gathers BF16 rows (opt-in mixed-precision propagation of the row-sharded step, llmrec_amd/dist_fused.py):
//   llmrec_rows_to_bf16      Xb[r] = RNE_bf16(row_scale[r] * X[r])                       one dense pass: the bf16 shadow of an fp32 tensor
//   llmrec_spmm_xbf16_f32    Y = post_scale . op(alpha Z + diag(rs) (P . val) diag(cs) widen(Xb)), optionally Yb = RNE_bf16(Y)
// What it is for: the SpMM at scale is bound by the fabric's rate for random row gathers (spmm.hip), and a d = 64 row is two 128-B lines
// in fp32 but one in bf16. Only the gathered operand is narrow: indices, weights, accumulators, epilogue operands and Y stay fp32.
// The kernels are the bodies of spmm_body.h instantiated for SpmmArgsXb - the fp32 vector families' lanes per row (d <= 16 / 32 / 64 /
// 128 / 256: 4 / 8 / 16 / 32 / 64 lanes, four columns each, now one 8-byte load widened by a 16-bit shift), the same four row buckets,
// permuted-CSR plans, pipelined short rows and prefetched indices, hence the same summation trees: the result is BIT-IDENTICAL to
// llmrec_spmm_f32 on the fp32 tensor widen(Xb). (Eight columns per lane - 16-byte loads, half the lanes per row - would change the
// wave / block / split trees and with them the bits; not built.)
// Unmasked products only: the masked, flagged and row-restricted products of the step gather few rows and stay fp32.
#include "common.h"
#include "spmm_body.h"
#include <string>

namespace llmrec {

template <int LPR, bool WEIGHTED>
__global__ __launch_bounds__(TPB) void spmm_xbf16_kernel(SpmmArgsXb a) {
    __shared__ __attribute__((aligned(16))) float red_lds[(TPB / 64 - 1) * LPR * 4];
    spmm_body<LPR, 1, 4, WEIGHTED, false>(a, (int32_t)blockIdx.x, red_lds);
}

// the split rows' second launch: it holds the finished row, so it is the one that writes their Yb
template <int LPR>
__global__ __launch_bounds__(256) void spmm_xbf16_finalize_kernel(SpmmArgsXb a) {
    __shared__ __attribute__((aligned(16))) float fin_lds[(256 / LPR) * LPR * 4];
    spmm_finalize_body<LPR, 1, 4>(a, (int32_t)blockIdx.x, fin_lds);
}

template <int LPR>
static int launch_spmm_xbf16(const SpmmArgsXb& a, bool weighted, int64_t total, hipStream_t stream) {
    if (total > 0) {
        if (weighted) spmm_xbf16_kernel<LPR, true><<<(unsigned)total, TPB, 0, stream>>>(a);
        else spmm_xbf16_kernel<LPR, false><<<(unsigned)total, TPB, 0, stream>>>(a);
        LLMREC_LAUNCH_CHECK();
    }
    if (a.n_split_rows > 0) {
        spmm_xbf16_finalize_kernel<LPR><<<(unsigned)a.n_split_rows, 256, 0, stream>>>(a);
        LLMREC_LAUNCH_CHECK();
    }
    return LLMREC_OK;
}

// one thread per VEC columns of a row, grid-stride; VEC = 4: float4 in, four bf16 (8 bytes) out
template <int VEC>
__global__ __launch_bounds__(256) void rows_to_bf16_kernel(int64_t n_rows, int32_t d, const float* __restrict__ row_scale, const float* __restrict__ X,
                                                           int64_t ldx, uint16_t* __restrict__ Xb, int64_t ldxb) {
    const int32_t per_row = d / VEC;
    const int64_t n = n_rows * per_row;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / per_row;
        const int32_t col = (int32_t)(i - r * per_row) * VEC;
        Vec<VEC> v;
        v.load(X + r * ldx + col);
        if (row_scale) v.scale(row_scale[r]);
        if constexpr (VEC == 4) v.store_bf16(Xb + r * ldxb + col);
        else Xb[r * ldxb + col] = (uint16_t)(rn_bf16_bits(v.v) >> 16);
    }
}

static bool ranges_overlap(const void* p, int64_t np, const void* q, int64_t nq) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return p && q && np > 0 && nq > 0 && a < b + (uintptr_t)nq && b < a + (uintptr_t)np;
}

}  // namespace llmrec

using namespace llmrec;

extern "C" int llmrec_rows_to_bf16(int64_t n_rows, int32_t d, const float* row_scale, const float* X, int64_t ldx, uint16_t* Xb, int64_t ldxb,
                                   llmrec_stream_t stream_) {
    LLMREC_CHECK_ARG(n_rows >= 0 && d >= 0, "rows_to_bf16: negative size");
    if (n_rows == 0 || d == 0) return LLMREC_OK;
    LLMREC_CHECK_ARG(X && Xb && ldx >= d && ldxb >= d, "rows_to_bf16: null pointer or ld < d");
    hipStream_t stream = (hipStream_t)stream_;
    const bool vec4 = d % 4 == 0 && ldx % 4 == 0 && ldxb % 4 == 0 && (uintptr_t)X % 16 == 0 && (uintptr_t)Xb % 8 == 0;
    if (vec4) rows_to_bf16_kernel<4><<<grid_for(n_rows * (d / 4), 256), 256, 0, stream>>>(n_rows, d, row_scale, X, ldx, Xb, ldxb);
    else rows_to_bf16_kernel<1><<<grid_for(n_rows * d, 256), 256, 0, stream>>>(n_rows, d, row_scale, X, ldx, Xb, ldxb);
    LLMREC_LAUNCH_CHECK();
    return LLMREC_OK;
}

extern "C" int llmrec_spmm_xbf16_f32(int64_t n_rows, int64_t n_cols, const int32_t* rowptr, const int32_t* colidx, const float* val,
                                     const float* row_scale, const float* col_scale, const uint16_t* Xb, int64_t ldxb, float* Y, int64_t ldy,
                                     uint16_t* Yb, int64_t ldyb, int32_t d, const llmrec_spmm_plan_t* plan_host, float* partials,
                                     const llmrec_spmm_epilogue_t* epilogue_host, llmrec_stream_t stream_) {
    LLMREC_CHECK_ARG(n_rows >= 0 && n_cols >= 0 && d >= 0, "spmm_xbf16: negative size");
    if (n_rows == 0 || d == 0) return LLMREC_OK;
    if (d % 4 != 0 || d > 256) {
        set_error("spmm_xbf16: d = %d outside the compiled kernel family (multiples of 4 up to 256)", d);
        return LLMREC_EUNSUPPORTED;
    }
    if (epilogue_host) {
        const llmrec_spmm_epilogue_t& e = *epilogue_host;
        if (e.x_row_mask || e.y_row_flag || e.z_row_flag || e.y_row_gate || e.y_row_needed || e.rows_listed_only || e.x_mask_stamp) {
            set_error("spmm_xbf16: compiled for the dense products only - a masked, flagged, gated or row-restricted product gathers few rows "
                      "and stays fp32 (llmrec_spmm_f32)");
            return LLMREC_EUNSUPPORTED;
        }
    }
    LLMREC_CHECK_ARG(rowptr && Y && Xb && ldy >= d && ldxb >= d, "spmm_xbf16: null pointer or ld < d");
    LLMREC_CHECK_ARG(ldxb % 4 == 0 && (uintptr_t)Xb % 8 == 0, "spmm_xbf16: the rows of Xb must be 8-byte aligned (ldxb a multiple of 4)");
    LLMREC_CHECK_ARG(!Yb || (ldyb >= d && ldyb % 4 == 0 && (uintptr_t)Yb % 8 == 0), "spmm_xbf16: the rows of Yb must be 8-byte aligned with ldyb >= d");
    LLMREC_CHECK_ARG(!Yb || !ranges_overlap(Yb, ((n_rows - 1) * ldyb + d) * 2, Xb, n_cols > 0 ? ((n_cols - 1) * ldxb + d) * 2 : 0),
                     "spmm_xbf16: Yb overlaps Xb (rows are gathered while others are written)");
    // everything else is llmrec_spmm_f32's: the plan, the epilogue, the fp32 operands' layout, the block ranges (X itself is not read)
    llmrec_spmm_problem_t pr = {n_rows, n_cols, rowptr, colidx, val, row_scale, col_scale, nullptr, ldxb, Y, ldy, d, 0, plan_host, partials, epilogue_host};
    SpmmSingle s;
    const int rc = spmm_prepare_single(pr, s);
    if (rc != LLMREC_OK) {
        const std::string why = llmrec_last_error();
        set_error("spmm_xbf16: %s", why.c_str());
        return rc;
    }
    LLMREC_CHECK_ARG(s.family <= 4, "spmm_xbf16: Y, Z, S and the partials must be 16-byte aligned rows (ld a multiple of 4): the fp32 vector path");
    SpmmArgsXb a;
    static_cast<SpmmArgs&>(a) = s.a;
    a.Xb = Xb; a.ldxb = ldxb; a.Yb = Yb; a.ldyb = ldyb;
    hipStream_t stream = (hipStream_t)stream_;
    switch (s.family) {
    case 0: return launch_spmm_xbf16<4>(a, s.weighted, s.blocks, stream);
    case 1: return launch_spmm_xbf16<8>(a, s.weighted, s.blocks, stream);
    case 2: return launch_spmm_xbf16<16>(a, s.weighted, s.blocks, stream);
    case 3: return launch_spmm_xbf16<32>(a, s.weighted, s.blocks, stream);
    default: return launch_spmm_xbf16<64>(a, s.weighted, s.blocks, stream);
    }
}
