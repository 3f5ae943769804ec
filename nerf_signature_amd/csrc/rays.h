// The ray through pixel centre (i, j) of a pinhole camera with the row-major [4,4] camera-to-world pose Pm (nerf/utils_wtmk_disen.py:131-137).  The ONE place the
// ray arithmetic is written: k_get_rays, both store samplers (write_sampled_ray) and the orbit sampler (raygen.hip) and the procedural scenes' ray caster
// (procedural.hip) call it, so their rays agree bit for bit.  Every includer is built with -ffp-contract=off (build.py): each operation is rounded on its own.
#pragma once
#include "common.h"

namespace nsig {
__device__ inline void pixel_ray(const float *__restrict__ Pm, float fx, float fy, float cx, float cy, float i, float j, float *__restrict__ o, float *__restrict__ d) {
    const float x = (i - cx) / fx, y = (j - cy) / fy, z = 1.0f;                               // (:131-133), zs == 1
    const float nrm = sqrtf(x * x + y * y + z * z);                                          // torch.norm(dim=-1)
    const float dx = x / nrm, dy = y / nrm, dz = z / nrm;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        d[r] = dx * Pm[4 * r] + dy * Pm[4 * r + 1] + dz * Pm[4 * r + 2];                      // directions @ R^T (:135)
        o[r] = Pm[4 * r + 3];                                                                // camera centre (:137)
    }
}
}  // namespace nsig
