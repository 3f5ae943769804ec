// Shared host/device helpers of libnerfsig (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <atomic>
#include <mutex>
#include <type_traits>

#include "../../include/nerfsig.h"

#define NSIG_EXPORT extern "C" __attribute__((visibility("default")))

namespace nsig {

constexpr int kWave = 64;         // CDNA wavefront
constexpr int kCUs = 256;         // MI355X
constexpr uint32_t kRowMask = NSIG_TABLE_ROWS - 1;

void set_error(const char *fmt, ...);
int check_launch(const char *what);

inline hipStream_t as_stream(nsig_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

#define NSIG_REQUIRE(cond, ...)           \
    do {                                  \
        if (!(cond)) {                    \
            nsig::set_error(__VA_ARGS__); \
            return NSIG_ERR_ARG;          \
        }                                 \
    } while (0)

__host__ __device__ inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
__host__ __device__ inline bool aligned8(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }
__host__ __device__ inline bool aligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

// A launch with more than 64 KB of dynamic LDS has to be allowed per kernel first.  `granted` is the call site's own record (a static std::atomic<size_t>, zero at
// start) of what `kernel` has been allowed so far; the attribute is set only when `bytes` exceeds it.  The entry points are reached from more than one thread
// (forward, autograd's backward): the record is read without a lock, and raised under one, so a kernel's limit never goes down.
template <typename K>
int reserve_lds(K kernel, size_t bytes, std::atomic<size_t> &granted, const char *who) {
    if (bytes <= granted.load(std::memory_order_acquire)) return NSIG_OK;
    static std::mutex raising;
    std::lock_guard<std::mutex> lock(raising);
    if (bytes <= granted.load(std::memory_order_relaxed)) return NSIG_OK;
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) {
        set_error("%s: cannot reserve %zu bytes of LDS", who, bytes);
        return NSIG_ERR_LAUNCH;
    }
    granted.store(bytes, std::memory_order_release);
    return NSIG_OK;
}

// Element i < n of K parallel host lists of device pointers into K arrays of a launch's argument struct, index by index: a null one is refused with null_fmt, one of
// the first `aligned` lists that is not 16-byte aligned with align_fmt (printf formats taking who and i).
template <typename T, size_t K>
int take_pointers(T *const (&dst)[K], T const *const (&src)[K], uint32_t n, const char *who, const char *null_fmt, const char *align_fmt = nullptr, size_t aligned = K) {
    for (uint32_t i = 0; i < n; ++i) {
        for (size_t k = 0; k < K; ++k) NSIG_REQUIRE(src[k][i] != nullptr, null_fmt, who, i);
        for (size_t k = 0; align_fmt && k < aligned; ++k) NSIG_REQUIRE(aligned16(src[k][i]), align_fmt, who, i);
        for (size_t k = 0; k < K; ++k) dst[k][i] = src[k][i];
    }
    return NSIG_OK;
}

// launch(std::true_type{}) or launch(std::false_type{}): a launch that differs in one bool template argument is written once, as a generic lambda (`decltype(flag)::value`).
template <typename Launch>
void with_flag(bool flag, Launch launch) {
    if (flag) launch(std::true_type{});
    else launch(std::false_type{});
}

__host__ __device__ inline uint32_t ceil_div(uint32_t a, uint32_t b) { return (a + b - 1) / b; }

__device__ inline float clampf(float v, float lo, float hi) { return fminf(hi, fmaxf(lo, v)); }

// d (grad_scale * mean of n squared differences) / d difference, per unit of difference: the seed factor of clean_loss and of rm_composite_train_mse
__host__ __device__ inline float mse_seed_factor(float grad_scale, uint32_t n) { return grad_scale * 2.0f / (float)n; }

// 10-bit-per-axis bit interleave (x -> bit 0, y -> bit 1, z -> bit 2 of every triple).
__host__ __device__ inline uint32_t spread3(uint32_t v) {
    v = (v * 0x00010001u) & 0xFF0000FFu;
    v = (v * 0x00000101u) & 0x0F00F00Fu;
    v = (v * 0x00000011u) & 0xC30C30C3u;
    v = (v * 0x00000005u) & 0x49249249u;
    return v;
}
__host__ __device__ inline uint32_t morton3(uint32_t x, uint32_t y, uint32_t z) {
    return spread3(x) | (spread3(y) << 1) | (spread3(z) << 2);
}
__host__ __device__ inline uint32_t compact3(uint32_t v) {
    v &= 0x49249249u;
    v = (v | (v >> 2)) & 0xc30c30c3u;
    v = (v | (v >> 4)) & 0x0f00f00fu;
    v = (v | (v >> 8)) & 0xff0000ffu;
    v = (v | (v >> 16)) & 0x0000ffffu;
    return v;
}

}  // namespace nsig
