// Wave and workgroup reductions and prefix sums of libnerfsig's kernels (device only).
// Every helper assumes workgroups made of whole 64-lane waves with all lanes active at the call.
#pragma once

#include "common.h"

namespace nsig {

// Reduction over the wave's 64 lanes, the result in every lane: the xor butterfly in the order 32, 16, 8, 4, 2, 1 (float results depend on that order).
template <typename T, typename Op>
__device__ __forceinline__ T wave_reduce(T v, Op op) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = op(v, __shfl_xor(v, d, 64));
    return v;
}
template <typename T>
__device__ __forceinline__ T wave_sum(T v) { return wave_reduce(v, [](T a, T b) { return a + b; }); }
template <typename T>
__device__ __forceinline__ T wave_max(T v) { return wave_reduce(v, [](T a, T b) { return max(a, b); }); }
template <typename T>
__device__ __forceinline__ T wave_min(T v) { return wave_reduce(v, [](T a, T b) { return min(a, b); }); }

// Inclusive scan over the wave's 64 lanes (`lane` = the caller's lane index): __shfl_up by 1, 2, .. 32.
template <typename T, typename Op>
__device__ __forceinline__ T wave_scan(T v, int lane, Op op) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T t = __shfl_up(v, d, 64);
        if (lane >= d) v = op(v, t);
    }
    return v;
}
template <typename T>
__device__ __forceinline__ T wave_prefix_sum(T v, int lane) { return wave_scan(v, lane, [](T a, T b) { return a + b; }); }

// Exclusive prefix sum of `mine` over a workgroup of kWaves waves in thread order; *total_out (optional) = the workgroup's sum, in every thread.
// All threads of the workgroup call it (one barrier inside); the caller places a barrier before it reuses wave_tot (LDS, kWaves words).
template <int kWaves, typename T>
__device__ __forceinline__ T block_exclusive_sum(T mine, T *wave_tot, T *total_out = nullptr) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const T incl = wave_prefix_sum(mine, lane);
    if (lane == 63) wave_tot[wid] = incl;
    __syncthreads();
    T before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        const T v = wave_tot[w];
        if (w < wid) before += v;
        total += v;
    }
    if (total_out != nullptr) *total_out = total;
    return before + incl - mine;
}

// Sum of `v` over the workgroup, in every thread: wave butterflies, then the waves in index order.  scratch: LDS, one float per wave;
// the leading barrier lets a caller pass the same scratch to consecutive calls.
__device__ __forceinline__ float block_sum(float v, float *scratch) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = 0.0f;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += scratch[w];
    return t;
}

}  // namespace nsig
