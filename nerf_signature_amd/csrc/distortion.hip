// The distortion layer's own kernels and entry points (include/nerfsig.h, wm_distort_*): the step's random draws, the layer alone, its adjoint (also the launch
// behind the fused decoder's image-gradient epilogue), and the two resampling kinds.  What they share with the decoder's first layer is distortion.h.
#include <algorithm>

#include "distortion.h"
#include "draws.h"

using namespace nsig;

// ---- the adjoint: one launch whatever the kind.
// gx (through the clamp) = clamp mask x the layer's adjoint applied to gy (the scratch image the decoder's epilogue left, or wm_distort_bwd's grad_out).  The kind is
// resolved first (a mixed set: the selector, the same word for every thread).  Every kind but the blur is pointwise.  The blur's adjoint is the transposed blur:
// gx[p] = sum over the (q, tap) whose reflected source is p of k[tap] * gy[q] -- one thread per (image, pixel, channel); the 3 x 3 outputs q around p are visited
// and each one's taps re-reflected.  Noise, none and the geometric kinds (whose resampling is a launch of its own) are the identity under the mask.
__global__ void __launch_bounds__(256) k_distort_adjoint(const float *__restrict__ gy, const float *__restrict__ img, Distortion d, uint32_t B, uint32_t Cin,
                                                         float *__restrict__ gx) {
    const uint32_t H = d.H, W = d.W, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B * H * W * Cin) return;
    const ResolvedKind r = resolve(d);
    if (r.kind != kDistBlur) {
        gx[i] = pointwise_adjoint(r.kind, r.param, img[i], gy[i]);
        return;
    }
    const uint32_t c = i % Cin, pix = (i / Cin) % (H * W), im = i / (Cin * H * W);
    const int y = (int)(pix / W), x = (int)(pix % W);
    float a, b;
    blur_taps(r.param[0], a, b);
    float acc = 0.0f;
    for (int qy = y - 2; qy <= y + 2; ++qy) {
        if (qy < 0 || qy >= (int)H) continue;
        float wy = 0.0f;          // total weight with which output row qy reads input row y (reflection can map two taps onto it)
        for (int dy = -1; dy <= 1; ++dy)
            if (reflect1(qy + dy, (int)H) == y) wy += dy == 0 ? b : a;
        if (wy == 0.0f) continue;
        for (int qx = x - 2; qx <= x + 2; ++qx) {
            if (qx < 0 || qx >= (int)W) continue;
            float wx = 0.0f;
            for (int dx = -1; dx <= 1; ++dx)
                if (reflect1(qx + dx, (int)W) == x) wx += dx == 0 ? b : a;
            if (wx != 0.0f) acc += wy * wx * gy[((size_t)im * H * W + (size_t)qy * W + qx) * Cin + c];
        }
    }
    const float v = img[i];
    gx[i] = (v >= 0.0f && v <= 1.0f) ? acc : 0.0f;
}

namespace nsig {
void launch_distort_adjoint(const float *gy, const float *img, const Distortion &d, uint32_t B, uint32_t C, float *gx, hipStream_t stream) {
    k_distort_adjoint<<<ceil_div(B * d.H * d.W * C, 256u), 256, 0, stream>>>(gy, img, d, B, C, gx);
}
}  // namespace nsig

// ---- the step's random draws, counter-based: everything is a function of (seed, *step, element) -- a replayed graph draws fresh values every step without a
// host-side generator.  Brightness factor U[0.5, 1.5], blur sigma U[0.01, 0.5], scaling factor 0.75 + 0.5 u (the factor the host draws for the same key,
// distortion.host_uniform; both are one rounding of the same sum), one angle per image, noise[i] ~ N(0, 0.1) (Box-Muller).  The hash is draws.h's 64-bit family
// under the key of (seed, step); the words outside the noise's indexed sequence finalise the key XORed with a constant of this file's own.
constexpr uint64_t kUnitXor = 0xFFFFFFFFFFFFFFFFull;          // the step's one uniform word: brightness, sigma, scaling factor
constexpr uint64_t kRotationMul = 0xA0761D6478BD642Full;      // image i's angle: key ^ (kRotationMul (i + 1))
constexpr uint64_t kSelectorXor = 0xC2B2AE3D27D4EB4Full;      // a mixed set's selector
__device__ inline float draw_unit(uint64_t key) { return unit24((uint32_t)(mix64(key ^ kUnitXor) >> 40)); }
// one angle in [-30, 30) degrees per image, stored as (cos, sin): param[2 i], param[2 i + 1]
__device__ inline void draw_rotation(uint64_t key, uint32_t i, float *__restrict__ param) {
    const float u = unit24((uint32_t)(mix64(key ^ (kRotationMul * ((uint64_t)i + 1ull))) >> 40));
    const float a = (60.0f * u - 30.0f) * 0.0174532925199432958f;
    param[2 * i] = cosf(a);
    param[2 * i + 1] = sinf(a);
}
__device__ inline float draw_noise(uint64_t key, uint32_t i) { return unit_normal(draw64(key, i), 0.316227766016837933f); }      // sigma = sqrt(0.1)
// Where the draw of a set (mask bit k = kind k) goes.  A mixed set: the words of its block.  A single kind, the one-member set: its parameter is param_out itself,
// there is no selector word (selector == nullptr) and no other kind's rotation pairs to keep at the identity (n_images = 0 unless rotation is the kind).
struct DrawDst {
    uint32_t *selector;
    float *brightness, *sigma, *scaling, *rotation, *noise;
    uint32_t n_images, n_noise;
};
// First WHICH kind this step trains against: the (floor(u n))-th member of the set (n members; a one-member set always picks that member), u a 24-bit word of
// a sequence of its own (distortion.host_selector is the host's statement of it).  Then that kind's parameter.  A block's rotation pairs are written EVERY step,
// (1, 0) unless rotation is selected: the resampling launch of a set that holds rotation is always enqueued, and at (1, 0) it copies.  The noise tensor is written
// only when noise is selected.  Every thread derives the selector itself (nothing is read back from the block); thread 0 stores it.
__global__ void __launch_bounds__(256) k_distort_draw(uint32_t mask, uint64_t seed, const uint32_t *__restrict__ step, DrawDst dst) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    const uint64_t key = stream_key(seed, step ? step[0] : 0u);
    uint32_t pick = (uint32_t)(((mix64(key ^ kSelectorXor) >> 40) * (uint64_t)__popc(mask)) >> 24), kind = 0;
    for (uint32_t k = 0; k <= kDistScaling; ++k)
        if ((mask >> k) & 1u) {
            if (pick == 0) {
                kind = k;
                break;
            }
            --pick;
        }
    if (i == 0) {
        if (dst.selector) dst.selector[0] = kind;
        const float u = draw_unit(key);
        if (kind == kDistBrightness) dst.brightness[0] = 0.5f + u;
        if (kind == kDistBlur) dst.sigma[0] = 0.01f + 0.49f * u;
        if (kind == kDistScaling) dst.scaling[0] = 0.75f + 0.5f * u;
    }
    if (i < dst.n_images) {
        if (kind == kDistRotation) {
            draw_rotation(key, i, dst.rotation);
        } else {
            dst.rotation[2 * i] = 1.0f;
            dst.rotation[2 * i + 1] = 0.0f;
        }
    }
    if (kind == kDistNoise && i < dst.n_noise) dst.noise[i] = draw_noise(key, i);
}

// the layer alone, [B][H][W][C] -> [B][H][W][C] (decoder shapes the fused chain does not implement; tests)
__global__ void __launch_bounds__(256) k_distort_fwd(const float *__restrict__ img, Distortion d, uint32_t B, uint32_t Cin, float *__restrict__ out) {
    const uint32_t P = d.H * d.W, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B * P * Cin) return;
    out[i] = distorted_value(img, d, i / (P * Cin), i % Cin, (i / Cin) % P, Cin, P);
}

// ---- the two kinds that change the sampling geometry (rotation, scaling): kernels of their own in front of / behind the decoder, which then reads their
// output as an ordinary rendered image (values in [0, 1]: its clamp is the identity and passes every gradient).
//
// rotation (torchvision RandomRotation((-30, 30)) per image: nearest-neighbour resampling about the centre, zeros outside, same size): the source of output
// pixel (x, y), measured from the centre ((W - 1) / 2, (H - 1) / 2), is round-half-even(cos * x - sin * y, sin * x + cos * y).  Every product and sum is
// rounded on its own (no fused multiply-add): the host-side statement of the same map (distortion.rotate_nearest) picks the same pixels bit for bit.
// At (cos, sin) = (1, 0) -- what a mixed set's draw leaves when another kind is selected -- the launch is an exact copy of clamp(img): xs = x - cx is exact
// (an integer minus a half-integer, both far below 2^23), 1 * xs = xs, 0 * ys = +-0, xs - +-0 = xs, and xs + cx = x exactly, so rintf gives (x, y) itself, always
// inside.  Its adjoint (k_distort_geom_bwd) then sums ONE term: its centre candidate round(1 * u + 0 * w + cx) is x itself, and of the 3 x 3 outputs around it each
// one's source is that output itself, so only q = p matches -- grad = 0 + gy[p], the clamp mask applied as in the decoder's own epilogue.
__device__ inline bool rotation_source(float c, float s, int x, int y, int H, int W, int &ix, int &iy) {
    const float cx = 0.5f * (float)(W - 1), cy = 0.5f * (float)(H - 1);
    const float xs = __fsub_rn((float)x, cx), ys = __fsub_rn((float)y, cy);
    const float sx = __fadd_rn(__fsub_rn(__fmul_rn(c, xs), __fmul_rn(s, ys)), cx);
    const float sy = __fadd_rn(__fadd_rn(__fmul_rn(s, xs), __fmul_rn(c, ys)), cy);
    ix = (int)rintf(sx);
    iy = (int)rintf(sy);
    return ix >= 0 && ix < W && iy >= 0 && iy < H;
}
// scaling (F.interpolate(image [3, H, W], scale_factor = sf, mode = 'linear'): 1-d, along W only, W_out = floor(W * sf), align_corners = False with the
// given factor kept for the coordinates): source position max(0, (xd + 0.5) / sf - 0.5), its two neighbours blended linearly -- except where W_out == W,
// which the operator special-cases as a plain copy whatever the factor (ATen upsample_linear1d: "special case: just copy")
__device__ inline void scaling_source(float rscale, int xd, int W, int Wo, int &x0, int &x1, float &l0, float &l1) {
    if (Wo == W) {
        x0 = x1 = xd;
        l0 = 1.0f;
        l1 = 0.0f;
        return;
    }
    float src = rscale * ((float)xd + 0.5f) - 0.5f;
    src = src < 0.0f ? 0.0f : src;
    x0 = (int)src;
    x0 = x0 > W - 1 ? W - 1 : x0;
    x1 = x0 + (x0 < W - 1 ? 1 : 0);
    l1 = src - (float)x0;
    l0 = 1.0f - l1;
}
__device__ inline float scaling_rscale(const float *__restrict__ param) { return (float)(1.0 / (double)param[0]); }

// out [B][H][Wo][C] = the layer on clamp(img [B][H][W][C]); clamped_out (optional) = clamp(img)
__global__ void __launch_bounds__(256) k_distort_geom_fwd(const float *__restrict__ img, uint32_t kind, const float *__restrict__ param, uint32_t B, uint32_t H,
                                                          uint32_t W, uint32_t Wo, uint32_t C, float *__restrict__ out, float *__restrict__ clamped_out) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (clamped_out && i < B * H * W * C) clamped_out[i] = clamp01(img[i]);
    if (i >= B * H * Wo * C) return;
    const uint32_t c = i % C, x = (i / C) % Wo, y = (i / (C * Wo)) % H, im = i / (C * Wo * H);
    const float *base = img + (size_t)im * H * W * C + c;
    if (kind == kDistRotation) {
        int ix, iy;
        out[i] = rotation_source(param[2 * im], param[2 * im + 1], (int)x, (int)y, (int)H, (int)W, ix, iy) ? clamp01(base[((size_t)iy * W + ix) * C]) : 0.0f;
    } else {
        int x0, x1;
        float l0, l1;
        scaling_source(scaling_rscale(param), (int)x, (int)W, (int)Wo, x0, x1, l0, l1);
        out[i] = l0 * clamp01(base[((size_t)y * W + x0) * C]) + l1 * clamp01(base[((size_t)y * W + x1) * C]);
    }
}
// grad_img [B][H][W][C] = the clamp's mask x the layer's adjoint applied to gy [B][H][Wo][C].  Gather form (one thread per source element, fixed summation
// order: deterministic).  rotation: an output pixel q reads source p only if |R^-1 q - p| <= 1/2 per axis, hence |q - R p| < 0.71: q lies in the 3 x 3
// neighbourhood of round(R p) -- each candidate's source is re-derived with the forward's own arithmetic.  scaling: every output column of the row is tried.
__global__ void __launch_bounds__(256) k_distort_geom_bwd(const float *__restrict__ gy, const float *__restrict__ img, uint32_t kind, const float *__restrict__ param,
                                                          uint32_t B, uint32_t H, uint32_t W, uint32_t Wo, uint32_t C, float *__restrict__ gx) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B * H * W * C) return;
    const uint32_t c = i % C, x = (i / C) % W, y = (i / (C * W)) % H, im = i / (C * W * H);
    const float v = img[i];
    if (!(v >= 0.0f && v <= 1.0f)) {
        gx[i] = 0.0f;
        return;
    }
    const float *g = gy + (size_t)im * H * Wo * C + c;
    float acc = 0.0f;
    if (kind == kDistRotation) {
        const float cs = param[2 * im], sn = param[2 * im + 1];
        const float cx = 0.5f * (float)(W - 1), cy = 0.5f * (float)(H - 1), u = (float)x - cx, w = (float)y - cy;
        const int qx0 = (int)rintf(cs * u + sn * w + cx), qy0 = (int)rintf(-sn * u + cs * w + cy);
        for (int qy = qy0 - 1; qy <= qy0 + 1; ++qy)
            for (int qx = qx0 - 1; qx <= qx0 + 1; ++qx) {
                if (qx < 0 || qx >= (int)W || qy < 0 || qy >= (int)H) continue;
                int ix, iy;
                if (rotation_source(cs, sn, qx, qy, (int)H, (int)W, ix, iy) && ix == (int)x && iy == (int)y) acc += g[((size_t)qy * Wo + qx) * C];
            }
    } else {
        const float rs = scaling_rscale(param);
        for (int xd = 0; xd < (int)Wo; ++xd) {
            int x0, x1;
            float l0, l1;
            scaling_source(rs, xd, (int)W, (int)Wo, x0, x1, l0, l1);
            const float gq = g[((size_t)y * Wo + xd) * C];
            if (x0 == (int)x) acc += l0 * gq;
            if (x1 == (int)x) acc += l1 * gq;
        }
    }
    gx[i] = acc;
}

// ---- entry points

// param_out: a single kind's parameter, or the mixed set's block -- then the set and the number of images travel in the code (NSIG_DISTORT_MIXED_CODE)
NSIG_EXPORT int wm_distort_draw(uint32_t distortion, uint64_t seed, const uint32_t *step_counter, uint32_t n_noise, float *param_out, float *noise_out,
                                nsig_stream_t stream) {
    NSIG_REQUIRE(distortion != kDistScaling, "wm_distort_draw: the scaling factor decides a tensor shape: the host draws it");
    Distortion d;
    const char *why = describe_distortion(d, distortion, param_out, noise_out, 2, 2, 1, 1u << kDistNoise | 1u << kDistBrightness | 1u << kDistBlur | 1u << kDistRotation);
    NSIG_REQUIRE(why == nullptr, "wm_distort_draw: %s", why);
    const bool mixed = is_mixed(d.code);
    const uint32_t mask = kinds_mask(d.code);
    auto has = [mask](uint32_t kind) { return ((mask >> kind) & 1u) != 0; };
    auto word = [&d](uint32_t kind) { return const_cast<float *>(param_of(d, kind)); };
    DrawDst dst{mixed ? reinterpret_cast<uint32_t *>(param_out) + NSIG_MIXED_SELECTOR : nullptr, word(kDistBrightness), word(kDistBlur), word(kDistScaling),
                word(kDistRotation), noise_out, mixed ? distortion >> 16 : (has(kDistRotation) ? n_noise : 0u), has(kDistNoise) ? n_noise : 0u};
    NSIG_REQUIRE(!has(kDistNoise) || n_noise >= 1, "wm_distort_draw: %s",
                 mixed ? "the mixed distortion's set holds noise: n_noise = the noise tensor's element count" : "noise draws n_noise elements (the noise tensor's element count)");
    NSIG_REQUIRE(!has(kDistRotation) || dst.n_images >= 1, "wm_distort_draw: %s",
                 mixed ? "the mixed distortion's set holds rotation: the code carries the number of images (NSIG_DISTORT_MIXED_CODE)"
                       : "rotation draws one angle per image (n_noise = the number of images)");
    const uint32_t n = std::max(std::max(dst.n_images, dst.n_noise), 1u);
    k_distort_draw<<<ceil_div(n, 256u), 256, 0, as_stream(stream)>>>(mask, seed, step_counter, dst);
    return check_launch("wm_distort_draw");
}

NSIG_EXPORT int wm_distort_fwd(const float *img, uint32_t B, uint32_t H, uint32_t W, uint32_t C, uint32_t distortion, const float *dist_param,
                               const float *dist_noise, float *out, nsig_stream_t stream) {
    NSIG_REQUIRE(img && out && B >= 1 && H >= 1 && W >= 1 && C >= 1 && (uint64_t)B * H * W * C < (1ull << 31), "wm_distort_fwd: bad arguments");
    Distortion d;
    const char *why = describe_distortion(d, distortion, dist_param, dist_noise, H, W, 1);
    NSIG_REQUIRE(why == nullptr, "wm_distort_fwd: %s", why);
    k_distort_fwd<<<ceil_div(B * H * W * C, 256u), 256, 0, as_stream(stream)>>>(img, d, B, C, out);
    return check_launch("wm_distort_fwd");
}

NSIG_EXPORT int wm_distort_bwd(const float *grad_out, const float *img, uint32_t B, uint32_t H, uint32_t W, uint32_t C, uint32_t distortion,
                               const float *dist_param, const float *dist_noise, float *grad_img, nsig_stream_t stream) {
    NSIG_REQUIRE(grad_out && img && grad_img && B >= 1 && H >= 1 && W >= 1 && C >= 1 && (uint64_t)B * H * W * C < (1ull << 31), "wm_distort_bwd: bad arguments");
    Distortion d;
    const char *why = describe_distortion(d, distortion, dist_param, dist_noise, H, W, 1);
    NSIG_REQUIRE(why == nullptr, "wm_distort_bwd: %s", why);
    launch_distort_adjoint(grad_out, img, d, B, C, grad_img, as_stream(stream));
    return check_launch("wm_distort_bwd");
}

NSIG_EXPORT int wm_distort_geom_fwd(const float *img, uint32_t B, uint32_t H, uint32_t W, uint32_t C, uint32_t distortion, const float *dist_param, uint32_t W_out,
                                    float *out, float *clamped_out, nsig_stream_t stream) {
    NSIG_REQUIRE(img && out && dist_param && B >= 1 && H >= 1 && W >= 1 && C >= 1 && W_out >= 1 && (uint64_t)B * H * (W > W_out ? W : W_out) * C < (1ull << 31),
                 "wm_distort_geom_fwd: bad arguments");
    NSIG_REQUIRE((distortion == kDistRotation && W_out == W) || distortion == kDistScaling,
                 "wm_distort_geom_fwd: distortion is 4 (rotation: W_out = W, dist_param = (cos, sin) per image) or 5 (scaling: dist_param[0] = the factor, W_out = floor(W * factor))");
    k_distort_geom_fwd<<<ceil_div(B * H * (W > W_out ? W : W_out) * C, 256u), 256, 0, as_stream(stream)>>>(img, distortion, dist_param, B, H, W, W_out, C, out, clamped_out);
    return check_launch("wm_distort_geom_fwd");
}

NSIG_EXPORT int wm_distort_geom_bwd(const float *grad_out, const float *img, uint32_t B, uint32_t H, uint32_t W, uint32_t C, uint32_t distortion,
                                    const float *dist_param, uint32_t W_out, float *grad_img, nsig_stream_t stream) {
    NSIG_REQUIRE(grad_out && img && grad_img && dist_param && B >= 1 && H >= 1 && W >= 1 && C >= 1 && W_out >= 1 &&
                     (uint64_t)B * H * (W > W_out ? W : W_out) * C < (1ull << 31),
                 "wm_distort_geom_bwd: bad arguments");
    NSIG_REQUIRE((distortion == kDistRotation && W_out == W) || distortion == kDistScaling, "wm_distort_geom_bwd: distortion is 4 (rotation, W_out = W) or 5 (scaling)");
    k_distort_geom_bwd<<<ceil_div(B * H * W * C, 256u), 256, 0, as_stream(stream)>>>(grad_out, img, distortion, dist_param, B, H, W, W_out, C, grad_img);
    return check_launch("wm_distort_geom_bwd");
}
