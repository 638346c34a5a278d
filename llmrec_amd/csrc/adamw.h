// adamw.h - THE AdamW update of one element, for every kernel that applies it: adamw_kernel, the multi-tensor launches and the
// row-sweep group (rowops.hip), and the update that rides in the weight-gradient reduction (dense.hip). They are compared bit for bit,
// so they share this one function instead of agreeing copy by copy.
#pragma once
#include "common.h"

namespace llmrec {

// p.mul_(1 - lr * wd)'s factor, rounded once from double: what every AdamW entry point passes to its kernel
static inline float adamw_decay_mul(float lr, float weight_decay) { return (float)(1.0 - (double)lr * (double)weight_decay); }

#ifdef __HIPCC__
struct AdamwConsts { float decay_mul, b2, eps, step_size, bc2s, w1, w2; };

// state: adamw_advance_kernel's [step count, lr / bias correction 1, sqrt(bias correction 2)]
__device__ __forceinline__ AdamwConsts adamw_consts(const float* __restrict__ state, float decay_mul, float b1, float b2, float eps) {
    AdamwConsts c;
    c.decay_mul = decay_mul; c.b2 = b2; c.eps = eps;
    c.step_size = state[1]; c.bc2s = state[2];
    c.w1 = 1.0f - b1; c.w2 = 1.0f - b2;
    return c;
}

// The update of one element (gi = the gradient the update uses). Contraction is OFF inside: the compiler fuses a * b + c into an fma
// where it pays - for the packed two-float instructions a float4 path is compiled to, not for scalar code, which rounds the product
// first. With it off every caller, packed or scalar, rounds the same way. Only the fmaf below is fused, everywhere.
__device__ __forceinline__ void adamw_element(const AdamwConsts& c, float gi, float& p, float& m, float& v) {
#pragma clang fp contract(off)
    float pi = p * c.decay_mul;                                    // p.mul_(1 - lr * wd)
    const float mi = m + c.w1 * (gi - m);                          // exp_avg.lerp_(grad, 1 - beta1)
    const float vi = fmaf(c.w2 * gi, gi, v * c.b2);                // mul_(beta2).addcmul_(g, g, 1 - beta2)
    const float denom = sqrtf(vi) / c.bc2s + c.eps;
    pi = pi - c.step_size * (mi / denom);                          // addcdiv_(exp_avg, denom, -step_size)
    p = pi; m = mi; v = vi;
}
// the gradient scaled by the caller's factor (1: untouched, not multiplied)
__device__ __forceinline__ float adamw_grad(float gs, float g) { return gs == 1.0f ? g : gs * g; }
#endif

}  // namespace llmrec
