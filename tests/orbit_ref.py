"""tests/orbit_ref.py -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Float64 mirror of the orbit sampler's draw and pose (csrc/draws.h: draw_base / draw_word; csrc/raygen.hip: orbit_pose, rg_sample_rays_orbit), and the bound the GPU
test holds `pose_out` to.  numpy only; imports nothing of the product.

The draw (tests/draw_ref.py states it in integers).  The counter hash of section 16: base = mix32(mix32(seed_lo ^ (k * 0x9e3779b9)) + seed_hi), a sequence s > 0 re-keys it as mix32(base + s * 0x7f4a7c15),
word i of a sequence is mix32(base ^ (i * 0x85ebca6b + 0x6b43a9b5)) -- all modulo 2^32.  The orbit pose of camera k = step * stride + offset takes words 0 and 1
of sequence 5 (0: uniform pixel indices, 1..3: the weighted sampler, 4: the RGBA backgrounds), each on torch.rand's grid: (word >> 8) * 2^-24.

The angles are fp32 quantities by definition -- theta = fl(fl(u (theta1 - theta0)) + theta0), the arithmetic of `torch.rand(n) * (hi - lo) + lo` in blocks.rand_poses --
so the mirror forms them in fp32 (IEEE: numpy's float32 operations round the same way) and everything after them in float64.

The bound (derived, not tuned).  An entry of the pose is +-1 trigonometric factor (rotation), a product of two (rotation), or the radius times one or two
(translation).  HIP's single-precision sinf and cosf are documented with a maximum error of 1 ulp over the full range (ROCm documentation, "HIP math API",
table "Single precision mathematical functions": sinf 1, cosf 1 -- the figures as published with ROCm 7.2, the release this project builds against; TRIG_ULP below
is that figure and follows it if a later release documents another; the same figures in the CUDA C Programming Guide's table the HIP table follows).  One ulp of a
result |t| <= 1 is at most 2^-23 |t| <= 2^-23 absolute.  With factors |t1|, |t2| <= 1 each off by at most TRIG_ULP 2^-23:
    |fl(t1' t2') - t1 t2|           <= 2 TRIG_ULP 2^-23 + (TRIG_ULP 2^-23)^2 + 2^-24 (one rounding of a product of magnitude <= 1 + 2^-22)
    |fl(fl(r t1') t2') - r t1 t2|   <= r (2 TRIG_ULP 2^-23 + 2 2^-24) (1 + 2^-20)     (the scale by the radius is one more rounded product)
so every entry is within  max(1, r) (2 TRIG_ULP 2^-23 + 2 2^-24) (1 + 2^-20)  of the mirror: POSE_BOUND(r).  The exact entries (0, 1) carry no error at all.
"""
import math

import numpy as np

from draw_ref import draw_base, draw_word, mix32, unit24      # noqa: F401 (the tests import the hashes from here)

M32 = 0xFFFFFFFF
ORBIT_SEQUENCE = 5
TRIG_ULP = 1.0          # documented maximum ulp error of HIP's sinf / cosf (see above)


def uniform24(word):
    """torch.rand's grid: 24 bits * 2^-24, exact in fp32."""
    return unit24(word >> 8)


def camera_index(step, stride, offset):
    return (step * stride + offset) & M32


def angles(seed, k, theta_range, phi_range):
    """(theta, phi) of camera k as the fp32 values the kernel forms (returned as Python floats: exactly representable)."""
    base = draw_base(seed, k, ORBIT_SEQUENCE)
    out = []
    for i, (lo, hi) in enumerate((theta_range, phi_range)):
        u, lo, hi = np.float32(uniform24(draw_word(base, i))), np.float32(lo), np.float32(hi)
        out.append(float(np.float32(np.float32(u * np.float32(hi - lo)) + lo)))
    return tuple(out)


def pose_from_angles(theta, phi, radius):
    """blocks.rand_poses' closed form in float64: right (-c_p, 0, s_p), up (c_t s_p, -s_t, c_t c_p), forward (-s_t s_p, -c_t, -s_t c_p), centre r (s_t s_p, c_t, s_t c_p)."""
    st, ct, sp, cp = math.sin(theta), math.cos(theta), math.sin(phi), math.cos(phi)
    r = float(np.float32(radius))
    return np.array([[-cp, ct * sp, -st * sp, r * st * sp],
                     [0.0, -st, -ct, r * ct],
                     [sp, ct * cp, -st * cp, r * st * cp],
                     [0.0, 0.0, 0.0, 1.0]], dtype=np.float64)


def pose(seed, step, stride, offset, radius, theta_range, phi_range):
    return pose_from_angles(*angles(seed, camera_index(step, stride, offset), theta_range, phi_range), radius)


def pose_bound(radius):
    """Largest |pose_out - mirror| any entry may show (see the module docstring)."""
    return max(1.0, float(radius)) * (2 * TRIG_ULP * 2.0 ** -23 + 2 * 2.0 ** -24) * (1 + 2.0 ** -20)


def pixel_indices(seed, step, n, H, W):
    """The N pixel indices of a step: sequence 0, word n scaled to [0, H * W) by the high half of a 64-bit product (k_sample_rays)."""
    base = draw_base(seed, step & M32, 0)
    return np.array([(draw_word(base, i) * (H * W)) >> 32 for i in range(n)], dtype=np.int64)
