// The counter hashes behind every random number a captured step draws: a draw is a pure function of (seed, a device counter, an element index), so a replayed
// graph draws fresh values without a host generator.  Two families, both stated here once and never merged (tests/draw_ref.py is the host's statement of
// both; tests/test_draw_ref_cpu.py holds it to known words).  A changed constant changes every training trajectory and fails no statistical test.
//   64 bits (splitmix64's finaliser): key = stream_key(seed, k), word i = draw64(key, i).  k is the distortion layer's step, stage 1's step + 1 (the NEXT
//     step's march offsets), the tamper noise's tensor index, the grid refresh's (refresh count, cascade, purpose).  A site that needs a word outside the
//     indexed sequence XORs its own constant into the key and finalises: mix64(key ^ constant); those constants stay at their sites.
//   32 bits (murmur3's finaliser): base = draw_base(seed_lo, seed_hi, step, stream), word i = draw_word(base, i): the ray samplers' streams of one step.
// A 24-bit word becomes a float on torch.rand's grid, exact in fp32: unit24 in [0, 1), unit24_open0 in (0, 1] (the argument of a logarithm).
#pragma once

#include "common.h"

namespace nsig {

__host__ __device__ inline uint64_t mix64(uint64_t z) {      // splitmix64's finaliser
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__host__ __device__ inline uint64_t stream_key(uint64_t seed, uint64_t k) { return mix64(seed ^ (0x9E3779B97F4A7C15ull * (k + 1ull))); }
__host__ __device__ inline uint64_t draw64(uint64_t key, uint64_t i) { return mix64(key + 0xD1B54A32D192ED03ull * (i + 1ull)); }

__host__ __device__ inline uint32_t mix32(uint32_t v) {      // murmur3's finaliser: full avalanche
    v ^= v >> 16; v *= 0x85ebca6bu; v ^= v >> 13; v *= 0xc2b2ae35u; v ^= v >> 16;
    return v;
}
// The streams of one step, independent sequences under the same (seed, step): the uniform samplers' pixel indices; the error-map race's cell keys and the
// pixel's row / column offsets inside its cell; the RGBA step's per-pixel background colours; the orbit sampler's two angles.
constexpr uint32_t kPixelStream = 0u, kRaceKeyStream = 1u, kRaceRowStream = 2u, kRaceColStream = 3u, kBackgroundStream = 4u, kOrbitStream = 5u;
// The per-step prefix of every draw: (seed, step) -> one word, re-keyed for a stream > 0.
__host__ __device__ inline uint32_t draw_base(uint32_t seed_lo, uint32_t seed_hi, uint32_t step, uint32_t stream) {
    const uint32_t b = mix32(mix32(seed_lo ^ (step * 0x9e3779b9u)) + seed_hi);
    return stream == 0u ? b : mix32(b + stream * 0x7f4a7c15u);
}
__host__ __device__ inline uint32_t draw_word(uint32_t base, uint32_t index) { return mix32(base ^ (index * 0x85ebca6bu + 0x6b43a9b5u)); }

__host__ __device__ inline float unit24(uint32_t word24) { return (float)word24 * (1.0f / 16777216.0f); }                 // [0, 1)
__host__ __device__ inline float unit24_open0(uint32_t word24) { return (float)(word24 + 1u) * (1.0f / 16777216.0f); }    // (0, 1]

// Box-Muller on one 64-bit word: the radius from bits 40..63, the angle from bits 8..31.  sigma scales the radius BEFORE the cosine is multiplied in, the
// order the distortion layer's noise has always had ((sigma r) cos, two roundings); at the default it is exact and the result is the unit normal.
__device__ inline float unit_normal(uint64_t h, float sigma = 1.0f) {
    const float u1 = unit24_open0((uint32_t)(h >> 40)), u2 = unit24((uint32_t)(h >> 8) & 0xFFFFFFu);
    return sigma * sqrtf(-2.0f * logf(u1)) * cosf(6.28318530717958648f * u2);
}

}  // namespace nsig
