// The plane set between the encoder (encode.hip) and the MLP kernels (field.hip, stage1*.hip): 17 feature planes of `stride` points, level-major, so that the
// stores of an encoder wave and the loads of an MLP half-wave are contiguous.  Two layouts:
//   fp32   planes[level][point] float2 -- every consumer reads it;
//   mixed  levels 0..14 as fp16 pairs (4 bytes per point), then level 15 and the codebook level as float2 -- written by hg_encode_planes_mixed for the fp16
//          MLP, whose first-layer operand is exactly those fp16 pairs (rounded to nearest even by the encoder instead of at the MLP's load: the same bits).  Level 15
//          stays fp32 because the codebook is added to it BEFORE the rounding (network_wtmk_tcnn.py:106).  15 x 4 + 2 x 8 = 76 instead of 136 bytes per point
//          each way between the encoder and the MLP.
// The OWNER of the buffer says which (NSIG_PLANES_F32 / NSIG_PLANES_MIXED) when it hands the set to an entry point that reads or completes it (`planes_layout`).
#pragma once

#include "mfma.h"

namespace nsig {

// points per plane: a multiple of 32, the MLP's tile (rows in [M, stride) replicate the last point and are never consumed)
__host__ __device__ inline uint32_t plane_stride(uint32_t M) { return ceil_div(M, 32u) * 32u; }

constexpr int kHalfLevels = NSIG_BASE_LEVELS - 1;
__device__ __host__ inline float2 *mixed_f32_plane(void *planes, uint32_t stride, int level) {      // level 15 or 16 of a mixed set
    return reinterpret_cast<float2 *>(reinterpret_cast<uint32_t *>(planes) + (size_t)kHalfLevels * stride) + (size_t)(level - kHalfLevels) * stride;
}
// where level l of point m goes; for l < kHalfLevels of a mixed set the address is that of a 4-byte fp16 pair
__device__ __host__ inline float2 *plane_dest(void *planes, uint32_t stride, bool mixed, int l, uint32_t m) {
    if (!mixed) return reinterpret_cast<float2 *>(planes) + (size_t)l * stride + m;
    if (l < kHalfLevels) return reinterpret_cast<float2 *>(reinterpret_cast<uint32_t *>(planes) + (size_t)l * stride + m);
    return mixed_f32_plane(planes, stride, l) + m;
}
__device__ inline float2 load_plane(const float2 *__restrict__ planes, uint32_t stride, int level, uint32_t s, bool mixed) {
    if (!mixed) return planes[(size_t)level * stride + s];
    if (level >= kHalfLevels) return mixed_f32_plane(const_cast<float2 *>(planes), stride, level)[s];
    const f32x2 w = __builtin_convertvector(__builtin_bit_cast(f16x2, reinterpret_cast<const uint32_t *>(planes)[(size_t)level * stride + s]), f32x2);
    return make_float2(w[0], w[1]);
}

inline int check_layout(int layout, const char *who) {
    NSIG_REQUIRE(layout == NSIG_PLANES_F32 || layout == NSIG_PLANES_MIXED, "%s: planes_layout must be NSIG_PLANES_F32 (0) or NSIG_PLANES_MIXED (1)", who);
    return NSIG_OK;
}
// K codebook planes beside one set of base planes (hg_encode_codebook_planes_multi writes them, field_fwd_multi reads them)
inline int check_multi_k(uint32_t K, const char *who) {
    NSIG_REQUIRE(K >= 1 && K <= NSIG_MULTI_MAX_MESSAGES, "%s: K=%u out of range [1,%d]", who, K, NSIG_MULTI_MAX_MESSAGES);
    return NSIG_OK;
}

}  // namespace nsig
