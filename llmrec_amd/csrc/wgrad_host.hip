// wgrad_host.hip - the multi-target weight gradient HOSTING one SpMM (llmrec_linear_wgrad_multi_adamw_host_spmm_bf16x3; the entry point,
// its checks and the reduction + AdamW launch behind this one are dense.hip's). A translation unit of its own: the kernel below is a
// second kernel around wgrad_bf16x3_v2_body, and compiled beside linear_wgrad_bf16x3_v2_multi_kernel it changes that kernel's
// instruction schedule (tools/isa_diff.py; profiles/experiments/r16_host_wgrad.md).
#include "wgrad_v2.h"

namespace llmrec {

// Blocks [0, wg_blocks) are linear_wgrad_bf16x3_v2_multi_kernel's, block for block (the XCD map over wg_blocks, not over the grid); the
// n_guest = gridDim.x - wg_blocks blocks behind them run the product's virtual blocks persistently, guest g the blocks g, g + n_guest,
// ... of a layout made for 256-thread blocks (spmm_hosted_body: every row keeps the summation tree of the 512-thread launch). A block
// of this kernel owns a CU (129 KB of LDS), the weight gradient's blocks are placed first, and the host launches no more blocks than the
// device has CUs: the guests land on the CUs the weight gradient's layout leaves free (llmrec_wgrad_target_t.block_budget). The loop is
// block-uniform and finite and no block waits for another, so a guest that finds no free CU simply runs behind a weight-gradient block.
// gridDim.y == 1 (N == 64). The product needs the first (TPB / 64 - 1) * 64 floats of red; the barrier keeps a virtual block's partial
// sums from the next one's.
__global__ __launch_bounds__(256, 1) void linear_wgrad_bf16x3_v2_multi_host_kernel(WgradMulti m, int N, int wg_blocks, SpmmArgs a) {
    __shared__ __attribute__((aligned(16))) float red[W2_RED_FLOATS];
    static_assert(W2_RED_FLOATS >= (TPB / 64 - 1) * 64, "the hosted product's partial sums fit the reduction array");
    if ((int)blockIdx.x < wg_blocks) {                               // (block-uniform)
        const int lb = xcd_logical_block(blockIdx.x, wg_blocks);
        int t = 0;
        while (t + 1 < m.n_targets && lb >= m.block_begin[t + 1]) ++t;
        wgrad_bf16x3_v2_body(m.g[t], N, m.K[t], m.partial[t], m.partial_db[t], m.MC, m.n_kslab[t], m.n_slabs[t], lb - m.block_begin[t], red);
        return;
    }
    const int64_t n_guest = (int64_t)gridDim.x - wg_blocks;
    for (int64_t vb = (int64_t)blockIdx.x - wg_blocks; vb < a.blk_end; vb += n_guest) {
        spmm_hosted_body<16, 1, 4, true, 256>(a, (int32_t)vb, red);
        __syncthreads();
    }
}

int wgrad_multi_host_launch(const WgradMulti& m, int N, int wg_blocks, int n_cu, const SpmmArgs& a, hipStream_t stream) {
    linear_wgrad_bf16x3_v2_multi_host_kernel<<<(unsigned)n_cu, 256, 0, stream>>>(m, N, wg_blocks, a);
    LLMREC_LAUNCH_CHECK();
    return LLMREC_OK;
}

}  // namespace llmrec
