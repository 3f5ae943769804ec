// Analytic scenes ray-cast into a uint8 image store (include/nerfsig.h, "procedural scenes"; restated in tests/procedural_ref.py).
//
// ps_render_u8: one lane per pixel of [P, H, W]; S x S sub-samples per pixel, K primitives per sub-sample, both loops with trip counts every lane shares.  The
// primitives, the light and the background travel in the launch's arguments: nothing is read from device memory but the poses, nothing is shared between lanes,
// nothing is allocated and no device value is read on the host.
// The ray is float32 -- rays.h's pixel_ray, the one every ray generator calls; tests/test_gpu_procedural.py compares with rg_get_rays -- and everything behind
// it is float64.  The library is built with -ffp-contract=off (build.py's BASE_FLAGS): every operation below is rounded on its own, in the order written.
#include "rays.h"

namespace nsig {

constexpr uint32_t kPsThreads = 256;                 // 4 waves
constexpr uint32_t kPsMaxSide = 4096;
constexpr double kPsTMin = NSIG_PROCEDURAL_T_MIN;

struct PsPrims {                                     // by value in the kernel's arguments: 1 KiB, read with scalar loads
    float v[NSIG_PROCEDURAL_MAX_PRIMS][NSIG_PROCEDURAL_PRIM_WORDS];
};
struct PsShade {
    float light[3], ambient, bg[3];
};

struct PsHit {
    double t;
    double n[3];
};

__device__ inline bool ps_sphere(const float *__restrict__ q, const double o[3], const double d[3], PsHit &h) {
    const double c0 = (double)q[4], c1 = (double)q[5], c2 = (double)q[6], r = (double)q[7];
    const double oc0 = o[0] - c0, oc1 = o[1] - c1, oc2 = o[2] - c2;
    const double A = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
    const double B = (oc0 * d[0] + oc1 * d[1]) + oc2 * d[2];
    const double Cq = ((oc0 * oc0 + oc1 * oc1) + oc2 * oc2) - r * r;
    const double disc = B * B - A * Cq;
    if (!(disc >= 0.0)) return false;
    const double s = sqrt(disc);
    double t = (-B - s) / A;
    if (!(t > kPsTMin)) t = (-B + s) / A;
    if (!(t > kPsTMin)) return false;
    h.t = t;
    h.n[0] = ((o[0] + t * d[0]) - c0) / r;
    h.n[1] = ((o[1] + t * d[1]) - c1) / r;
    h.n[2] = ((o[2] + t * d[2]) - c2) / r;
    return true;
}

__device__ inline bool ps_box(const float *__restrict__ q, const double o[3], const double d[3], PsHit &h) {
    double tn = -INFINITY, tf = INFINITY;
    int an = 0, af = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double lo = (double)q[4 + k], hi = (double)q[7 + k];
        if (d[k] == 0.0) {
            if (o[k] < lo || o[k] > hi) return false;
            continue;
        }
        const double t0 = (lo - o[k]) / d[k], t1 = (hi - o[k]) / d[k];
        const double nr = d[k] > 0.0 ? t0 : t1, fr = d[k] > 0.0 ? t1 : t0;
        if (nr > tn) tn = nr, an = k;                // a tie stays with the lower axis
        if (fr < tf) tf = fr, af = k;
    }
    if (!(tn <= tf) || !(tf > kPsTMin)) return false;
    const bool outside = tn > kPsTMin;
    const int ax = outside ? an : af;
    h.t = outside ? tn : tf;
#pragma unroll
    for (int k = 0; k < 3; ++k) h.n[k] = k == ax ? (d[k] > 0.0 ? -1.0 : 1.0) : 0.0;
    return true;
}

__global__ void __launch_bounds__(kPsThreads) k_ps_render_u8(const float *__restrict__ poses, uint32_t npix, float fx, float fy, float cx, float cy, uint32_t H, uint32_t W,
                                                             const PsPrims prims, uint32_t K, const PsShade sh, uint32_t S, uint32_t C, uint8_t *__restrict__ image) {
    const uint32_t g = blockIdx.x * kPsThreads + threadIdx.x;
    if (g >= npix) return;
    const uint32_t hw = H * W, p = g / hw, pix = g % hw, i = pix % W, j = pix / W;
    const float *Pm = poses + 16 * (size_t)p;
    const double l0 = (double)sh.light[0], l1 = (double)sh.light[1], l2 = (double)sh.light[2];
    const double len = sqrt((l0 * l0 + l1 * l1) + l2 * l2);
    const double L0 = l0 / len, L1 = l1 / len, L2 = l2 / len;
    const double amb = (double)sh.ambient, dif = 1.0 - amb;
    const float twoS = (float)(2u * S);
    double sum[3] = {0.0, 0.0, 0.0};
    uint32_t hits = 0;
    for (uint32_t b = 0; b < S; ++b) {
        for (uint32_t a = 0; a < S; ++a) {
            const float u = (float)i + (float)(2u * a + 1u) / twoS, v = (float)j + (float)(2u * b + 1u) / twoS;      // exact for S in {1, 2, 4}
            float of[3], df[3];
            pixel_ray(Pm, fx, fy, cx, cy, u, v, of, df);
            const double o[3] = {(double)of[0], (double)of[1], (double)of[2]}, d[3] = {(double)df[0], (double)df[1], (double)df[2]};
            PsHit best;
            best.t = INFINITY;
            best.n[0] = best.n[1] = best.n[2] = 0.0;
            uint32_t win = K;
            for (uint32_t k = 0; k < K; ++k) {
                const float *q = prims.v[k];
                PsHit h;
                const bool hit = q[0] == 0.0f ? ps_sphere(q, o, d, h) : ps_box(q, o, d, h);
                if (hit && h.t < best.t) best = h, win = k;      // equal t stays with the lower index
            }
            if (win == K) continue;
            const float *q = prims.v[win];
            bool odd = false;
            if (q[1] != 0.0f) {
                const double f = (double)q[2];
                const long long n = (long long)floor(f * (o[0] + best.t * d[0])) + (long long)floor(f * (o[1] + best.t * d[1])) + (long long)floor(f * (o[2] + best.t * d[2]));
                odd = (n & 1ll) != 0;
            }
            const double nl = (best.n[0] * L0 + best.n[1] * L1) + best.n[2] * L2;
            const double shade = amb + dif * fmax(0.0, nl);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) sum[ch] = sum[ch] + (double)(odd ? q[13 + ch] : q[10 + ch]) * shade;
            ++hits;
        }
    }
    const double alpha = (double)hits / (double)(S * S);
    uint8_t *out = image + (size_t)g * C;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        double c = hits ? sum[ch] / (double)hits : 0.0;
        if (C == 3) c = c * alpha + (double)sh.bg[ch] * (1.0 - alpha);
        out[ch] = (uint8_t)rint(255.0 * fmin(1.0, fmax(0.0, c)));      // round half to even
    }
    if (C == 4) out[3] = (uint8_t)rint(255.0 * alpha);
}

static inline bool ps_finite(float v) { return fabsf(v) <= 3.402823466e38f; }      // false for NaN and infinity

}  // namespace nsig

using namespace nsig;

NSIG_EXPORT int ps_render_u8(const float *poses, uint32_t P, float fx, float fy, float cx, float cy, uint32_t H, uint32_t W, const float *prims_host, uint32_t K,
                             float light_x, float light_y, float light_z, float ambient, uint32_t samples, uint32_t channels, float bg_r, float bg_g, float bg_b,
                             uint8_t *image, nsig_stream_t stream) {
    NSIG_REQUIRE(H >= 1 && H <= kPsMaxSide && W >= 1 && W <= kPsMaxSide, "ps_render_u8: image of %u x %u pixels is out of range (1 .. 4096 each way)", H, W);
    NSIG_REQUIRE(P >= 1 && (uint64_t)P * H * W < (1ull << 32), "ps_render_u8: P=%u views of %u x %u pixels out of range (P >= 1, P H W < 2^32)", P, H, W);
    NSIG_REQUIRE(K <= NSIG_PROCEDURAL_MAX_PRIMS, "ps_render_u8: K=%u primitives out of range (0 .. 16)", K);
    NSIG_REQUIRE(samples == 1 || samples == 2 || samples == 4, "ps_render_u8: samples=%u is not 1, 2 or 4", samples);
    NSIG_REQUIRE(channels == 3 || channels == 4, "ps_render_u8: channels=%u is not 3 or 4", channels);
    NSIG_REQUIRE(poses && image && (prims_host || K == 0), "ps_render_u8: null pointer");
    NSIG_REQUIRE(ps_finite(fx) && ps_finite(fy) && ps_finite(cx) && ps_finite(cy) && fx != 0.0f && fy != 0.0f,
                 "ps_render_u8: the intrinsics must be finite and the focal lengths non-zero");
    NSIG_REQUIRE(ps_finite(light_x) && ps_finite(light_y) && ps_finite(light_z) && (light_x != 0.0f || light_y != 0.0f || light_z != 0.0f),
                 "ps_render_u8: the light must be a finite vector other than zero");
    NSIG_REQUIRE(ambient >= 0.0f && ambient <= 1.0f, "ps_render_u8: ambient=%g outside [0, 1]", (double)ambient);
    NSIG_REQUIRE(ps_finite(bg_r) && ps_finite(bg_g) && ps_finite(bg_b), "ps_render_u8: the background must be finite");
    PsPrims prims = {};
    for (uint32_t k = 0; k < K; ++k) {
        const float *q = prims_host + NSIG_PROCEDURAL_PRIM_WORDS * (size_t)k;
        for (uint32_t w = 0; w < NSIG_PROCEDURAL_PRIM_WORDS; ++w) {
            NSIG_REQUIRE(ps_finite(q[w]), "ps_render_u8: primitive %u: word %u is not finite", k, w);
            prims.v[k][w] = q[w];
        }
        NSIG_REQUIRE(q[0] == 0.0f || q[0] == 1.0f, "ps_render_u8: primitive %u: kind %g is neither 0 (sphere) nor 1 (box)", k, (double)q[0]);
        NSIG_REQUIRE(q[1] == 0.0f || q[1] == 1.0f, "ps_render_u8: primitive %u: texture %g is neither 0 (flat) nor 1 (checker)", k, (double)q[1]);
        if (q[0] == 0.0f) {
            NSIG_REQUIRE(q[7] > 0.0f, "ps_render_u8: primitive %u: radius %g is not > 0", k, (double)q[7]);
        } else {
            for (uint32_t a = 0; a < 3; ++a) NSIG_REQUIRE(q[4 + a] <= q[7 + a], "ps_render_u8: primitive %u: box lo > hi on axis %u", k, a);
        }
    }
    const PsShade sh = {{light_x, light_y, light_z}, ambient, {bg_r, bg_g, bg_b}};
    const uint32_t npix = P * H * W;
    k_ps_render_u8<<<(npix - 1) / kPsThreads + 1, kPsThreads, 0, as_stream(stream)>>>(poses, npix, fx, fy, cx, cy, H, W, prims, K, sh, samples, channels, image);
    return check_launch("ps_render_u8");
}
