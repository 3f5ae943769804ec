// Model tampering on the device: what somebody who holds a released model's weights does to them -- magnitude pruning, parameter noise, uniform
// quantisation, fp16 storage -- as one pass from a pristine copy into the live tensors, plus the two reductions the pass needs: per-tensor statistics and
// the exact k-th smallest magnitude over ALL listed values together (the arithmetic is restated in tests/tamper_ref.py).
//
// Tensor lists: host arrays of device pointers and element counts, any n >= 1, launched in groups of at most 32 tensors (the launch argument holds
// 32 pointers); a tensor of 0 elements takes part in nothing.  Nothing reads a device value on the host; every launch is stream-ordered.
//   statistics: pass 1 -- tensor t's nb_t <= 256 workgroups stride over it and store (min, max, sum, count) of its finite elements, double; the finish
//               launch adds the nb_t partials in a fixed order (thread i holds partial i; wave butterfly, waves in index order) -> min, max, mean;
//               pass 2 -- sum (x - mean)^2 the same way -> the unbiased deviation.  No atomics: the same inputs give the same bits.
//   select:     radix select on the 31 magnitude bits m = bits & 0x7fffffff (monotone in |x|; NaN above infinity) in three passes of 11, 10 and 10
//               bits, most significant first.  Pass p: at most 256 workgroups walk the 4096-element chunks of the whole list (a workgroup takes chunks
//               b, b + 256, ...); elements whose bits above the pass's digit equal the prefix found so far count into the workgroup's LDS histogram
//               (integer LDS atomics), which is then merged, non-empty bins only, into the pass's global histogram (integer global atomics: the sums
//               do not depend on the order).  One workgroup then picks the bin that holds the remaining rank and leaves the longer prefix, the rank
//               inside the bin and the count below the bin in device memory for the next pass.  No sort, no copy of the data: three reads of it.
//   apply:      one workgroup per 4096 elements, 16-byte accesses where both tensors allow them; src == dst is allowed (every element is read once,
//               then written once, by the same thread).
// No float atomics anywhere.  The file is compiled with -ffp-contract=off like the rest of the library: no product and sum below contract, and no
// flag swaps logf / sqrtf / cosf or the division for native approximations.
#include <math.h>

#include "draws.h"

namespace nsig {

constexpr int kTmGroup = 32;                   // tensors per launch
constexpr uint32_t kTmChunk = 4096;            // elements per chunk
constexpr uint32_t kTmStatThreads = 256, kTmStatBlocks = 256;      // per tensor at most 256 partials: one per thread of the finish launch
constexpr uint32_t kTmSelThreads = 1024, kTmSelBlocks = 256;       // the select: one float4 per thread per chunk, one workgroup per CU
constexpr uint32_t kTmApplyThreads = 256;
constexpr int kTmPasses = 3;
constexpr uint32_t kTmBins = 2048;             // of the widest pass (bits 30..20; then 19..10 and 9..0: 1024 bins)

struct TmList {
    const float *src[kTmGroup];
    float *dst[kTmGroup];
    uint32_t numel[kTmGroup], chunk0[kTmGroup + 1];      // chunk0: first workgroup (statistics) or chunk (select, apply) of tensor i
};

// scratch: part[n][256][4] double (min, max, sum -- later the squared sum --, count), then the select's area
struct TmSelect {
    unsigned long long hist[kTmPasses][kTmBins];
    unsigned long long rank, below;      // 1-based rank inside the prefix's bin; values strictly below the prefix
    uint32_t prefix, pad;
};
static inline size_t tm_align(size_t b) { return (b + 255) & ~size_t(255); }
static inline size_t tm_part_bytes(uint32_t n) { return tm_align(size_t(n) * kTmStatBlocks * 4 * sizeof(double)); }
static inline TmSelect *tm_select_area(void *scratch, uint32_t n) { return reinterpret_cast<TmSelect *>(static_cast<char *>(scratch) + tm_part_bytes(n)); }

__device__ inline bool tm_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// the tensor (uniform) that owns position `at` of a launch's chunk table
__device__ inline uint32_t tm_owner(const uint32_t *chunk0, uint32_t n, uint32_t at) {
    uint32_t i = 0;
    while (i + 1 < n && at >= chunk0[i + 1]) ++i;
    return i;
}

// Sum over a workgroup of 256 threads in a fixed order (wave butterfly 32 .. 1, then the waves in index order); valid in thread 0.
__device__ inline double tm_block_sum(double v, double *red) {
    const uint32_t tid = threadIdx.x;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    double s = 0.0;
    if (tid == 0) {
#pragma unroll
        for (uint32_t w = 0; w < kTmStatThreads / kWave; ++w) s += red[w];
    }
    __syncthreads();
    return s;
}
__device__ inline double tm_block_min(double v, double *red) {
    const uint32_t tid = threadIdx.x;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fmin(v, __shfl_xor(v, d, 64));
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    double s = v;
    if (tid == 0) {
#pragma unroll
        for (uint32_t w = 0; w < kTmStatThreads / kWave; ++w) s = fmin(s, red[w]);
    }
    __syncthreads();
    return s;
}

// ----------------------------------------------------------------------------- statistics

// SECOND = false: (min, max, sum, count) of the finite elements; true: the sum of (x - mean)^2 over them, into slot 2.  first: list index of a.src[0].
template <bool SECOND>
__global__ void __launch_bounds__(kTmStatThreads) k_tm_stats_pass(TmList a, uint32_t n, uint32_t first, const double *__restrict__ stats,
                                                                  double *__restrict__ part) {
    __shared__ double red[kTmStatThreads / kWave];
    const uint32_t t = tm_owner(a.chunk0, n, blockIdx.x), b = blockIdx.x - a.chunk0[t], nb = a.chunk0[t + 1] - a.chunk0[t], numel = a.numel[t];
    const float *__restrict__ x = a.src[t];
    double *slot = part + ((size_t)(first + t) * kTmStatBlocks + b) * 4;
    if (SECOND) {
        const double mean = stats[(size_t)(first + t) * 4 + 2];
        double ss = 0.0;
        for (uint64_t i = (uint64_t)b * kTmStatThreads + threadIdx.x; i < numel; i += (uint64_t)nb * kTmStatThreads) {
            const float v = x[i];
            if (tm_finite(v)) {
                const double d = (double)v - mean;
                ss += d * d;
            }
        }
        ss = tm_block_sum(ss, red);
        if (threadIdx.x == 0) slot[2] = ss;
    } else {
        double lo = INFINITY, hi = -INFINITY, sum = 0.0, cnt = 0.0;
        for (uint64_t i = (uint64_t)b * kTmStatThreads + threadIdx.x; i < numel; i += (uint64_t)nb * kTmStatThreads) {
            const float v = x[i];
            if (tm_finite(v)) {
                lo = fmin(lo, (double)v);
                hi = fmax(hi, (double)v);
                sum += (double)v;
                cnt += 1.0;
            }
        }
        lo = tm_block_min(lo, red);
        hi = -tm_block_min(-hi, red);
        sum = tm_block_sum(sum, red);
        cnt = tm_block_sum(cnt, red);
        if (threadIdx.x == 0) {
            slot[0] = lo; slot[1] = hi; slot[2] = sum; slot[3] = cnt;
        }
    }
}

// Workgroup t: tensor first + t.  A tensor without a finite element gets (0, 0, 0, 0); one finite element gives a deviation of 0.
template <bool SECOND>
__global__ void __launch_bounds__(kTmStatThreads) k_tm_stats_finish(TmList a, uint32_t first, const double *__restrict__ part, double *__restrict__ stats) {
    __shared__ double red[kTmStatThreads / kWave];
    const uint32_t t = blockIdx.x, nb = a.chunk0[t + 1] - a.chunk0[t], tid = threadIdx.x;
    const double *slot = part + ((size_t)(first + t) * kTmStatBlocks + tid) * 4;
    double *out = stats + (size_t)(first + t) * 4;
    const bool mine = tid < nb;
    const double cnt = tm_block_sum(mine ? slot[3] : 0.0, red);
    const double sum = tm_block_sum(mine ? slot[2] : 0.0, red);
    if (SECOND) {
        if (tid == 0) out[3] = cnt > 1.0 ? sqrt(sum / (cnt - 1.0)) : 0.0;
    } else {
        const double lo = tm_block_min(mine ? slot[0] : (double)INFINITY, red), hi = -tm_block_min(mine ? -slot[1] : (double)INFINITY, red);
        if (tid == 0) {
            out[0] = cnt > 0.0 ? lo : 0.0;
            out[1] = cnt > 0.0 ? hi : 0.0;
            out[2] = cnt > 0.0 ? sum / cnt : 0.0;
            out[3] = 0.0;
        }
    }
}

// ----------------------------------------------------------------------------- select

__global__ void __launch_bounds__(256) k_tm_select_begin(TmSelect *__restrict__ s, unsigned long long k) {
    unsigned long long *h = &s->hist[0][0];
    for (uint32_t i = threadIdx.x; i < kTmPasses * kTmBins; i += 256) h[i] = 0ull;
    if (threadIdx.x == 0) {
        s->rank = k;
        s->below = 0ull;
        s->prefix = 0u;
    }
}

template <int PASS>
__device__ __forceinline__ void tm_count(uint32_t bits, uint32_t prefix, uint32_t *hist) {
    constexpr uint32_t shift = PASS == 0 ? 20u : (PASS == 1 ? 10u : 0u), width = PASS == 0 ? 11u : 10u;
    const uint32_t m = bits & 0x7fffffffu;
    if (PASS == 0 || (m >> (shift + width)) == (prefix >> (shift + width))) atomicAdd(&hist[(m >> shift) & ((1u << width) - 1u)], 1u);
}

template <int PASS>
__global__ void __launch_bounds__(kTmSelThreads) k_tm_select_hist(TmList a, uint32_t n, TmSelect *__restrict__ s) {
    __shared__ uint32_t hist[kTmBins];
    constexpr uint32_t bins = PASS == 0 ? 2048u : 1024u;
    const uint32_t tid = threadIdx.x, chunks = a.chunk0[n];
    for (uint32_t i = tid; i < bins; i += kTmSelThreads) hist[i] = 0u;
    const uint32_t prefix = PASS == 0 ? 0u : s->prefix;
    __syncthreads();
    for (uint32_t c = blockIdx.x; c < chunks; c += gridDim.x) {      // (c is uniform)
        const uint32_t t = tm_owner(a.chunk0, n, c), numel = a.numel[t];
        const uint32_t head = (c - a.chunk0[t]) * kTmChunk, tail = numel - head < kTmChunk ? numel : head + kTmChunk;      // (head < numel: a chunk exists only below numel)
        const float *__restrict__ x = a.src[t];
        if (aligned16(x) && tail - head == kTmChunk) {
            const uint4 v = *reinterpret_cast<const uint4 *>(x + head + 4u * tid);
            tm_count<PASS>(v.x, prefix, hist);
            tm_count<PASS>(v.y, prefix, hist);
            tm_count<PASS>(v.z, prefix, hist);
            tm_count<PASS>(v.w, prefix, hist);
        } else {
            for (uint32_t i = head + tid; i < tail; i += kTmSelThreads) tm_count<PASS>(__float_as_uint(x[i]), prefix, hist);
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i < bins; i += kTmSelThreads) {
        const uint32_t c = hist[i];
        if (c) atomicAdd(&s->hist[PASS][i], (unsigned long long)c);
    }
}

// One workgroup: the bin of pass PASS that holds the remaining rank.  After the last pass the prefix is the answer: *threshold_bits, and
// *count_le = the values below it + the values equal to it.
template <int PASS>
__global__ void __launch_bounds__(256) k_tm_select_pick(TmSelect *__restrict__ s, uint32_t *__restrict__ threshold_bits, unsigned long long *__restrict__ count_le) {
    __shared__ unsigned long long sums[256];
    constexpr uint32_t bins = PASS == 0 ? 2048u : 1024u, per = bins / 256u, shift = PASS == 0 ? 20u : (PASS == 1 ? 10u : 0u);
    const unsigned long long *h = s->hist[PASS];
    unsigned long long mine = 0ull;
    for (uint32_t j = 0; j < per; ++j) mine += h[threadIdx.x * per + j];
    sums[threadIdx.x] = mine;
    __syncthreads();
    if (threadIdx.x != 0) return;
    unsigned long long rank = s->rank, before = 0ull;      // 1 <= rank <= the histogram's total: the host checked k, every pass keeps it so
    uint32_t g = 0;
    while (g + 1 < 256u && before + sums[g] < rank) before += sums[g++];
    uint32_t b = g * per;
    while (b + 1 < (g + 1) * per && before + h[b] < rank) before += h[b++];
    s->prefix |= b << shift;
    s->rank = rank - before;
    s->below += before;
    if (PASS == kTmPasses - 1) {
        *threshold_bits = s->prefix;
        *count_le = s->below + h[b];
    }
}

// ----------------------------------------------------------------------------- apply

struct TmScalars {      // per tensor of the launch, read from the statistics by the kernel itself
    float s, lo, step;
    bool pass;          // quantise: a constant tensor passes through
};

template <uint32_t KIND>
__device__ __forceinline__ float tm_value(float x, uint32_t j, uint32_t threshold, uint64_t key, const TmScalars &c, float L) {
    if (KIND == NSIG_TAMPER_PRUNE) return (__float_as_uint(x) & 0x7fffffffu) <= threshold ? 0.0f : x;
    if (KIND == NSIG_TAMPER_NOISE) return x + c.s * unit_normal(draw64(key, j));      // word j of the key of (seed, tensor): draws.h
    if (KIND == NSIG_TAMPER_QUANTIZE) {
        if (c.pass || !tm_finite(x)) return x;
        const float q = fminf(L, fmaxf(0.0f, rintf((x - c.lo) / c.step)));
        return c.lo + q * c.step;
    }
    return (float)(_Float16)x;
}

template <uint32_t KIND>
__global__ void __launch_bounds__(kTmApplyThreads) k_tm_apply(TmList a, uint32_t n, uint32_t first, float strength, uint32_t bits,
                                                              const uint32_t *__restrict__ threshold_bits, const double *__restrict__ stats, uint64_t seed) {
    const uint32_t t = tm_owner(a.chunk0, n, blockIdx.x), numel = a.numel[t];
    const uint32_t head = (blockIdx.x - a.chunk0[t]) * kTmChunk, tail = numel - head < kTmChunk ? numel : head + kTmChunk;
    const float *x = a.src[t];      // (not __restrict__: src may be dst)
    float *y = a.dst[t];
    const uint32_t threshold = KIND == NSIG_TAMPER_PRUNE ? *threshold_bits : 0u;
    const uint64_t key = KIND == NSIG_TAMPER_NOISE ? stream_key(seed, first + t) : 0ull;
    const float L = (float)((1u << bits) - 1u);
    TmScalars c{0.0f, 0.0f, 1.0f, false};
    if (KIND == NSIG_TAMPER_NOISE) c.s = (float)((double)strength * stats[(size_t)(first + t) * 4 + 3]);
    if (KIND == NSIG_TAMPER_QUANTIZE) {
        const float lo = (float)stats[(size_t)(first + t) * 4], hi = (float)stats[(size_t)(first + t) * 4 + 1];
        c.lo = lo;
        c.step = (hi - lo) / L;
        c.pass = hi == lo;
    }
    if (aligned16(x) && aligned16(y) && tail - head == kTmChunk) {
        for (uint32_t i = head + 4u * threadIdx.x; i < tail; i += 4u * kTmApplyThreads) {
            float4 v = *reinterpret_cast<const float4 *>(x + i);
            v.x = tm_value<KIND>(v.x, i, threshold, key, c, L);
            v.y = tm_value<KIND>(v.y, i + 1u, threshold, key, c, L);
            v.z = tm_value<KIND>(v.z, i + 2u, threshold, key, c, L);
            v.w = tm_value<KIND>(v.w, i + 3u, threshold, key, c, L);
            *reinterpret_cast<float4 *>(y + i) = v;
        }
    } else {
        for (uint32_t i = head + threadIdx.x; i < tail; i += kTmApplyThreads) y[i] = tm_value<KIND>(x[i], i, threshold, key, c, L);
    }
}

// The groups of a list: checks first (nothing is launched for a list that is refused), then `launch(list, count, first index)` per group of <= 32 tensors
// with at least one element.  per_chunk: elements per position of chunk0; cap: at most this many positions per tensor (0 = no cap).
static int tm_check_list(const char *who, const float *const *src_host, float *const *dst_host, const uint32_t *numel_host, uint32_t n, bool with_dst) {
    NSIG_REQUIRE(src_host && numel_host && (!with_dst || dst_host), "%s: null pointer", who);
    NSIG_REQUIRE(n >= 1, "%s: the tensor list is empty (n = 0)", who);
    for (uint32_t i = 0; i < n; ++i)
        NSIG_REQUIRE(numel_host[i] == 0 || (src_host[i] && aligned4(src_host[i]) && (!with_dst || (dst_host[i] && aligned4(dst_host[i])))),
                     "%s: tensor %u has a null or misaligned pointer", who, i);
    return NSIG_OK;
}
static TmList tm_group(const float *const *src_host, float *const *dst_host, const uint32_t *numel_host, uint32_t first, uint32_t cnt, uint32_t per_chunk, uint32_t cap) {
    TmList a{};
    for (uint32_t i = 0; i < cnt; ++i) {
        const uint32_t j = first + i;
        a.src[i] = src_host[j];
        a.dst[i] = dst_host ? dst_host[j] : nullptr;
        a.numel[i] = numel_host[j];
        const uint32_t c = (uint32_t)(((uint64_t)numel_host[j] + per_chunk - 1) / per_chunk);
        a.chunk0[i + 1] = a.chunk0[i] + (cap && c > cap ? cap : c);
    }
    return a;
}

}  // namespace nsig

using namespace nsig;

NSIG_EXPORT size_t tm_scratch_bytes(uint32_t n) {
    if (n < 1) return 0;
    return tm_part_bytes(n) + tm_align(sizeof(TmSelect));
}

NSIG_EXPORT int tm_stats(const float *const *src_host, const uint32_t *numel_host, uint32_t n, double *stats, void *scratch, nsig_stream_t stream) {
    if (int e = tm_check_list("tm_stats", src_host, nullptr, numel_host, n, false)) return e;
    NSIG_REQUIRE(stats && scratch, "tm_stats: null pointer");
    NSIG_REQUIRE(aligned16(scratch) && aligned8(stats), "tm_stats: scratch must be 16-byte aligned, stats 8-byte aligned");
    hipStream_t st = as_stream(stream);
    double *part = static_cast<double *>(scratch);
    for (uint32_t first = 0; first < n; first += kTmGroup) {
        const uint32_t cnt = n - first < (uint32_t)kTmGroup ? n - first : (uint32_t)kTmGroup;
        const TmList a = tm_group(src_host, nullptr, numel_host, first, cnt, kTmChunk, kTmStatBlocks);
        if (a.chunk0[cnt]) k_tm_stats_pass<false><<<a.chunk0[cnt], kTmStatThreads, 0, st>>>(a, cnt, first, stats, part);
        k_tm_stats_finish<false><<<cnt, kTmStatThreads, 0, st>>>(a, first, part, stats);
        if (a.chunk0[cnt]) k_tm_stats_pass<true><<<a.chunk0[cnt], kTmStatThreads, 0, st>>>(a, cnt, first, stats, part);
        k_tm_stats_finish<true><<<cnt, kTmStatThreads, 0, st>>>(a, first, part, stats);
        if (int e = check_launch("tm_stats")) return e;
    }
    return NSIG_OK;
}

template <int PASS>
static int tm_select_pass(const float *const *src_host, const uint32_t *numel_host, uint32_t n, TmSelect *sel, uint32_t *threshold_bits,
                          unsigned long long *count_le, hipStream_t st) {
    for (uint32_t first = 0; first < n; first += kTmGroup) {
        const uint32_t cnt = n - first < (uint32_t)kTmGroup ? n - first : (uint32_t)kTmGroup;
        const TmList a = tm_group(src_host, nullptr, numel_host, first, cnt, kTmChunk, 0);
        const uint32_t chunks = a.chunk0[cnt];
        if (chunks) k_tm_select_hist<PASS><<<chunks < kTmSelBlocks ? chunks : kTmSelBlocks, kTmSelThreads, 0, st>>>(a, cnt, sel);
    }
    k_tm_select_pick<PASS><<<1, 256, 0, st>>>(sel, threshold_bits, count_le);
    return check_launch("tm_abs_kth");
}

NSIG_EXPORT int tm_abs_kth(const float *const *src_host, const uint32_t *numel_host, uint32_t n, uint64_t k, uint32_t *threshold_bits, uint64_t *count_le,
                           void *scratch, nsig_stream_t stream) {
    if (int e = tm_check_list("tm_abs_kth", src_host, nullptr, numel_host, n, false)) return e;
    NSIG_REQUIRE(threshold_bits && count_le && scratch, "tm_abs_kth: null pointer");
    NSIG_REQUIRE(aligned16(scratch) && aligned8(count_le), "tm_abs_kth: scratch must be 16-byte aligned, count_le 8-byte aligned");
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; ++i) total += numel_host[i];
    NSIG_REQUIRE(k >= 1 && k <= total, "tm_abs_kth: k = %llu is out of range (1 .. %llu, the number of listed values)", (unsigned long long)k, (unsigned long long)total);
    hipStream_t st = as_stream(stream);
    TmSelect *sel = tm_select_area(scratch, n);
    unsigned long long *le = reinterpret_cast<unsigned long long *>(count_le);
    k_tm_select_begin<<<1, 256, 0, st>>>(sel, (unsigned long long)k);
    if (int e = tm_select_pass<0>(src_host, numel_host, n, sel, threshold_bits, le, st)) return e;
    if (int e = tm_select_pass<1>(src_host, numel_host, n, sel, threshold_bits, le, st)) return e;
    return tm_select_pass<2>(src_host, numel_host, n, sel, threshold_bits, le, st);
}

NSIG_EXPORT int tm_apply(const float *const *src_host, float *const *dst_host, const uint32_t *numel_host, uint32_t n, uint32_t kind, float strength, uint32_t bits,
                         const uint32_t *threshold_bits, const double *stats, uint64_t seed, nsig_stream_t stream) {
    if (int e = tm_check_list("tm_apply", src_host, dst_host, numel_host, n, true)) return e;
    NSIG_REQUIRE(kind <= NSIG_TAMPER_HALF, "tm_apply: unknown kind %u (0 prune, 1 noise, 2 quantize, 3 half)", kind);
    NSIG_REQUIRE(strength >= 0.0f && strength <= 3.402823466e38f, "tm_apply: the strength must be a finite number >= 0");
    NSIG_REQUIRE(kind != NSIG_TAMPER_QUANTIZE || (bits >= 2 && bits <= 16), "tm_apply: quantize to %u bits is out of range (2 .. 16)", bits);
    NSIG_REQUIRE(kind != NSIG_TAMPER_PRUNE || threshold_bits, "tm_apply: prune needs the threshold (threshold_bits, tm_abs_kth's)");
    NSIG_REQUIRE((kind != NSIG_TAMPER_NOISE && kind != NSIG_TAMPER_QUANTIZE) || stats, "tm_apply: noise and quantize need the statistics (stats, tm_stats')");
    hipStream_t st = as_stream(stream);
    if (kind != NSIG_TAMPER_QUANTIZE) bits = 2;
    for (uint32_t first = 0; first < n; first += kTmGroup) {
        const uint32_t cnt = n - first < (uint32_t)kTmGroup ? n - first : (uint32_t)kTmGroup;
        const TmList a = tm_group(src_host, dst_host, numel_host, first, cnt, kTmChunk, 0);
        const uint32_t grid = a.chunk0[cnt];
        if (!grid) continue;
        switch (kind) {
            case NSIG_TAMPER_PRUNE: k_tm_apply<NSIG_TAMPER_PRUNE><<<grid, kTmApplyThreads, 0, st>>>(a, cnt, first, strength, bits, threshold_bits, stats, seed); break;
            case NSIG_TAMPER_NOISE: k_tm_apply<NSIG_TAMPER_NOISE><<<grid, kTmApplyThreads, 0, st>>>(a, cnt, first, strength, bits, threshold_bits, stats, seed); break;
            case NSIG_TAMPER_QUANTIZE: k_tm_apply<NSIG_TAMPER_QUANTIZE><<<grid, kTmApplyThreads, 0, st>>>(a, cnt, first, strength, bits, threshold_bits, stats, seed); break;
            default: k_tm_apply<NSIG_TAMPER_HALF><<<grid, kTmApplyThreads, 0, st>>>(a, cnt, first, strength, bits, threshold_bits, stats, seed); break;
        }
        if (int e = check_launch("tm_apply")) return e;
    }
    return NSIG_OK;
}
