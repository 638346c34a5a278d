// dropout.hip - llmrec_dropout_rows_f32: in-place inverted dropout of a row-major [rows, cols] view (reference Models.py:145-150,
// nn.Dropout on the eight projections) with a counter-based mask - a pure function of (seed, step, tensor tag, row, column), stated in
// full on the declaration (include/llmrec_hip.h). The fused step launches it on the projections behind the projection launch and, with the
// same masks, on their gradients ahead of the weight gradients; nothing launches it at rate 0.
//
// Memory-bound elementwise work: one Philox4x32-10 call (guests.h: the sampler's generator, another key) gives the four words of four
// consecutive columns, so a lane owns one float4. A block is a (256 >> shift) rows x (1 << shift) column-groups tile - 1 << shift = the
// power of two >= the row's groups, 256 at most - so (row, group) needs no division, and walks the rows grid-stride; rows wider than 256
// groups are walked by the tile's lanes. Element offsets are 64-bit. No LDS, no scratch, no float atomics.
//
// The step counter is device memory, so a replayed graph follows it. A launch with a ticket word counts its blocks off on it after their
// last read of the counter (the count-off of llmrec_sample_batch_wide, guests.h): the block that draws the last ticket advances the counter
// and puts the ticket back to 0. Nobody waits for anybody.
#include "common.h"
#include "guests.h"
#include <math.h>

namespace llmrec {

constexpr uint64_t DROPOUT_KEY = 0xD1B54A32D192ED03ull;              // seed ^ this: a stream of its own beside the sampler's two keys

__device__ __forceinline__ float drop1(float x, uint32_t word, uint32_t T, float scale) { return word >= T ? x * scale : 0.f; }

// VEC: the base is 16-byte aligned and ldx % 4 == 0, so every whole column group is one aligned float4
template <bool VEC>
__global__ __launch_bounds__(256) void dropout_rows_kernel(int64_t rows, int cols, int groups, int shift, float* X, int64_t ldx, uint32_t T,
                                                           float scale, uint64_t key, unsigned long long* step_dev, uint32_t tag,
                                                           int32_t* ticket) {
    const unsigned long long step = *step_dev;
    const uint32_t c2 = (uint32_t)step, c3 = (uint32_t)(step >> 32) * 256u + tag;
    const Philox ph(key);
    const int lanes = 1 << shift, g0 = threadIdx.x & (lanes - 1);
    const int64_t rows_per_block = 256 >> shift;
    for (int64_t r = (int64_t)blockIdx.x * rows_per_block + (threadIdx.x >> shift); r < rows; r += (int64_t)gridDim.x * rows_per_block) {
        float* __restrict__ row = X + r * ldx;
        for (int g = g0; g < groups; g += lanes) {
            const int c = 4 * g;                                        // groups <= 2^29: no overflow
            uint32_t o[4];
            ph((uint32_t)g, (uint32_t)r, c2, c3, o);
            if (VEC && cols - c >= 4) {
                float4 v = *reinterpret_cast<const float4*>(row + c);
                v.x = drop1(v.x, o[0], T, scale); v.y = drop1(v.y, o[1], T, scale);
                v.z = drop1(v.z, o[2], T, scale); v.w = drop1(v.w, o[3], T, scale);
                *reinterpret_cast<float4*>(row + c) = v;
            } else {                                                    // guarded: columns [cols, ldx) are never touched
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k < cols - c) row[c + k] = drop1(row[c + k], o[k], T, scale);
            }
        }
    }
    if (ticket == nullptr) return;                                      // (uniform) the launch only reads the counter
    __syncthreads();                                                    // every thread of this block is done with the step's value
    if (threadIdx.x == 0) {
        __threadfence();
        if (atomicAdd(ticket, 1) == (int)gridDim.x - 1) {               // the last block: every block has read the counter
            *step_dev = step + 1ull;
            atomicExch(ticket, 0);
        }
    }
}

}  // namespace llmrec

using namespace llmrec;

extern "C" {

int llmrec_dropout_rows_f32(int64_t rows, int32_t cols, float* X, int64_t ldx, float p, uint64_t seed, uint64_t* step_dev,
                            int32_t tensor_tag, int32_t* ticket, llmrec_stream_t stream_) {
    LLMREC_CHECK_ARG(p > 0.f && p < 1.f, "dropout_rows: p = %g outside (0, 1)", (double)p);      // (false for a NaN)
    LLMREC_CHECK_ARG(cols >= 1 && rows >= 0 && rows < (1ll << 32), "dropout_rows: bad sizes");
    LLMREC_CHECK_ARG(tensor_tag >= 0 && tensor_tag < 256, "dropout_rows: tensor_tag %d outside [0, 256)", (int)tensor_tag);
    if (rows == 0) return LLMREC_OK;
    LLMREC_CHECK_ARG(X && step_dev && ldx >= cols, "dropout_rows: null pointer or ld < cols");
    LLMREC_CHECK_ARG(((uintptr_t)X & 3) == 0, "dropout_rows: X is not 4-byte aligned");
    long long t = llrint((double)p * 4294967296.0);
    t = t < 1 ? 1 : (t > 0xffffffffll ? 0xffffffffll : t);
    const float scale = 1.0f / (1.0f - p);
    const int groups = (cols - 1) / 4 + 1;
    int shift = 0;
    while (shift < 8 && (1 << shift) < groups) ++shift;
    const int grid = grid_for(rows, 256 >> shift);
    const bool vec = ((uintptr_t)X & 15) == 0 && ldx % 4 == 0;
    auto kernel = vec ? dropout_rows_kernel<true> : dropout_rows_kernel<false>;
    kernel<<<grid, 256, 0, (hipStream_t)stream_>>>(rows, cols, groups, shift, X, ldx, (uint32_t)t, scale, seed ^ DROPOUT_KEY,
                                                   (unsigned long long*)step_dev, (uint32_t)tensor_tag, ticket);
    LLMREC_LAUNCH_CHECK();
    return LLMREC_OK;
}

}  // extern "C"
