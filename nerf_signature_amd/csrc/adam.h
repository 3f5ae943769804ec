// torch.optim.Adam's arithmetic (no weight decay / amsgrad: main_nerf_wtmk.py:110, main_nerf.py:122), once, and what the passes built on it share: optim.hip's codebook and
// dense passes, and the scatter owners' epilogue of hg_levels_scatter_adam in hashgrid.hip.
#pragma once

#include "common.h"

namespace nsig {

// torch.optim.Adam's update of one element
__device__ inline void adam_update(float g, float &p, float &m, float &v, float beta1, float beta2, float eps, float step_size, float inv_bc2_sqrt) {
    m = m + (1.0f - beta1) * (g - m);                 // exp_avg.lerp_(grad, 1 - beta1)
    v = v * beta2 + ((1.0f - beta2) * g) * g;         // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    const float denom = sqrtf(v) * inv_bc2_sqrt + eps;  // (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)
    p = p - step_size * (m / denom);                  // param.addcdiv_(exp_avg, denom, value=-step_size)
}

// ... of the four elements of a 16-byte vector, in .x .y .z .w order; grad_scale: for a gradient that is yet to be scaled
__device__ inline void adam_update4(const float4 &g, float4 &p, float4 &m, float4 &v, float beta1, float beta2, float eps, float step_size, float inv_bc2_sqrt,
                                    float grad_scale = 1.0f) {
    adam_update(g.x * grad_scale, p.x, m.x, v.x, beta1, beta2, eps, step_size, inv_bc2_sqrt);
    adam_update(g.y * grad_scale, p.y, m.y, v.y, beta1, beta2, eps, step_size, inv_bc2_sqrt);
    adam_update(g.z * grad_scale, p.z, m.z, v.z, beta1, beta2, eps, step_size, inv_bc2_sqrt);
    adam_update(g.w * grad_scale, p.w, m.w, v.w, beta1, beta2, eps, step_size, inv_bc2_sqrt);
}

// The two scalars of step t that adam_update takes, into a prepare kernel's scratch: [i] = lr / (1 - beta1^t), [stride + i] = 1 / sqrt(1 - beta2^t).
// beta^t as exp(t * log(beta)) in double: same value to ~1e-13 relative, a fraction of pow()'s latency in these one-workgroup kernels
__device__ __forceinline__ void adam_step_scalars(float step, const float *__restrict__ lr, float beta1, float beta2, float *__restrict__ scratch, uint32_t i, uint32_t stride) {
    scratch[i] = (float)((double)*lr / (1.0 - exp((double)step * log((double)beta1))));
    scratch[stride + i] = (float)(1.0 / sqrt(1.0 - exp((double)step * log((double)beta2))));
}

// The dense passes step kAdamGroup tensors per group of launches, and that is their scratch's stride.  adam_prepare_launch (optim.hip): step counts + 1 and the scratch
// of n <= kAdamGroup tensors, one launch of k_adam_dense_prepare -- also what hg_levels_scatter_adam's owners read.
constexpr int kAdamGroup = 32;
int adam_prepare_launch(float *const *steps_host, uint32_t n, const float *lr, float beta1, float beta2, float *scratch, hipStream_t st, const char *who);

// Streaming accesses of the optimiser passes: 836 MiB go through once per step; marked non-temporal so that they do not displace the
// base tables (64 MiB) from the L2 / Infinity Cache right before the next step's gather.
typedef float nsig_f32x4 __attribute__((ext_vector_type(4)));
template <bool NT>
__device__ __forceinline__ float4 ld4(const float4 *p) {
    if (!NT) return *p;
    const nsig_f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const nsig_f32x4 *>(p));
    return make_float4(v.x, v.y, v.z, v.w);
}
template <bool NT>
__device__ __forceinline__ void st4(float4 *p, const float4 &a) {
    if (!NT) {
        *p = a;
        return;
    }
    const nsig_f32x4 v = {a.x, a.y, a.z, a.w};
    __builtin_nontemporal_store(v, reinterpret_cast<nsig_f32x4 *>(p));
}

// Tensor i of a multi-tensor launch has the workgroups chunk0[i] .. chunk0[i + 1] - 1: the tensor workgroup `block` serves (uniform)
__device__ inline uint32_t chunk_owner(const uint32_t *chunk0, uint32_t n, uint32_t block) {
    uint32_t i = 0;
    while (i + 1 < n && block >= chunk0[i + 1]) ++i;
    return i;
}
__device__ inline uint32_t chunk_owner(const uint32_t *chunk0, uint32_t n) { return chunk_owner(chunk0, n, blockIdx.x); }

}  // namespace nsig
