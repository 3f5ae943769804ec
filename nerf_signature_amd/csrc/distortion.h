// The distortion layer of the training step (Trainer.distortion_layer, utils_wtmk_disen.py:551-577, applied at :594 between the clamp and the normalisation):
// what the decoder's first layer (decoder_fused.hip) and the layer's own kernels (distortion.hip) share.
//
// 0 none; 1 noise: x + noise[b][y][x][c] (the reference draws N(0, 0.1) per element); 2 brightness: clamp(f * x, 0, 1) (torchvision ColorJitter(brightness=0.5):
// ONE factor f in [0.5, 1.5] per call, blended against black); 3 blurring: the 3x3 Gaussian of torchvision GaussianBlur(3, sigma in [0.01, 0.5]) -- taps
// exp(-0.5 (d / sigma)^2), d in {-1, 0, 1}, normalised, reflect padding; 4 rotation and 5 scaling change the sampling geometry and are launches of their own
// (k_distort_geom_fwd / _bwd).  f / sigma are read from device memory (so a captured step can draw them itself), the noise from the noise tensor.
// 6 mixed (code = 6 | the set's mask << 8): the kind itself is a word in device memory -- param is the block of include/nerfsig.h (selector, then every kind's
// parameter at its own word).  A single kind is the one-member case: its kind is the code and its parameter sits at word 0.  resolve() says which, once per call
// (the same words for every lane: scalar loads); every per-kind statement below then exists once.
#pragma once
#include "common.h"

namespace nsig {

enum : uint32_t { kDistNone = 0, kDistNoise = 1, kDistBrightness = 2, kDistBlur = 3, kDistRotation = 4, kDistScaling = 5, kDistMixed = NSIG_DISTORT_MIXED };
constexpr uint32_t kDistAllKinds = 0x3Fu;      // the bits a mixed set's mask may hold: one per kind 0..5
constexpr uint32_t kDistFusedKinds = 0x0Fu;    // the kinds a single code may name where the layer is applied on load: 0..3

struct Distortion {
    uint32_t code, H, W;             // code: a single kind, or 6 | mask << 8
    const float *param, *noise;      // the kind's parameter word(s) or the mixed set's block; the noise tensor [B][H][W][C]
};

__host__ __device__ inline bool is_mixed(uint32_t code) { return (code & 0xFFu) == kDistMixed; }
// the set a code names, one bit per kind: a mixed code carries it, a single kind is the set of itself
__host__ __device__ inline uint32_t kinds_mask(uint32_t code) { return is_mixed(code) ? (code >> 8) & 0xFFu : (code <= kDistScaling ? 1u << code : 0u); }
// where `kind` keeps its parameter: word 0 of a single kind's param, its own word of a mixed set's block
__host__ __device__ inline const float *param_of(const Distortion &d, uint32_t kind) {
    if (!is_mixed(d.code)) return d.param;
    return d.param + (kind == kDistBrightness ? NSIG_MIXED_BRIGHTNESS : (kind == kDistBlur ? NSIG_MIXED_SIGMA : (kind == kDistScaling ? NSIG_MIXED_SCALING : NSIG_MIXED_ROTATION)));
}

// this step's kind of a mixed set.  The host checked what every member of the mask needs (a noise tensor, two pixels for the blur), so a selector word that
// names no member of the set -- a block nobody has drawn into yet -- reads as "none" instead of reaching for a buffer that may not be there
__device__ inline uint32_t mixed_selector(uint32_t code, const float *__restrict__ block) {
    const uint32_t sel = reinterpret_cast<const uint32_t *>(block)[NSIG_MIXED_SELECTOR];
    return (sel <= kDistScaling && ((code >> (8 + sel)) & 1u)) ? sel : (uint32_t)kDistNone;
}
struct ResolvedKind {
    uint32_t kind;
    const float *param;      // what the kind's statements read as param[0]
};
__device__ inline ResolvedKind resolve(const Distortion &d) {
    const uint32_t kind = is_mixed(d.code) ? mixed_selector(d.code, d.param) : d.code;
    return {kind, param_of(d, kind)};
}

__device__ inline float clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }
__device__ inline int reflect1(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }   // torch 'reflect' padding by one (n >= 2)
// side weight a and centre weight b of the normalised 1-d kernel [a, b, a]
__device__ inline void blur_taps(float sigma, float &a, float &b) {
    const float e = __expf(-0.5f / (sigma * sigma));
    b = 1.0f / (1.0f + 2.0f * e);
    a = e * b;
}

// the distorted value of channel c at pixel pix of image im, from the rendered blocks [B][H][W][Cin] (before the normalisation); 4, 5 and 0: the clamped value
__device__ inline float distorted_value(const float *__restrict__ img, const Distortion &d, uint32_t im, uint32_t c, uint32_t pix, uint32_t Cin, uint32_t P) {
    const float *base = img + (size_t)im * P * Cin + c;
    const ResolvedKind r = resolve(d);
    if (r.kind == kDistBlur) {
        float a, b;
        blur_taps(r.param[0], a, b);
        const int y = (int)(pix / d.W), x = (int)(pix - (uint32_t)y * d.W);
        float acc = 0.0f;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
            const int yy = reflect1(y + dy, (int)d.H);
            float row = 0.0f;
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) row += (dx == 0 ? b : a) * clamp01(base[(size_t)(yy * (int)d.W + reflect1(x + dx, (int)d.W)) * Cin]);
            acc += (dy == 0 ? b : a) * row;
        }
        return acc;
    }
    const float x = clamp01(base[(size_t)pix * Cin]);
    if (r.kind == kDistNoise) return x + d.noise[((size_t)im * P + pix) * Cin + c];
    if (r.kind == kDistBrightness) return clamp01(r.param[0] * x);
    return x;
}

// d loss / d (unclamped render) at one element of a kind that touches no neighbour (every kind but the blur), from g = d loss / d (distorted value): the
// brightness factor where f * clamp(x) stays inside [0, 1], then the clamp's mask (the gradient passes where 0 <= x <= 1, as torch.clamp)
__device__ inline float pointwise_adjoint(uint32_t kind, const float *__restrict__ param, float x, float g) {
    if (kind == kDistBrightness) {
        const float f = param[0], fx = f * clamp01(x);
        g = (fx >= 0.0f && fx <= 1.0f) ? g * f : 0.0f;
    }
    return (x >= 0.0f && x <= 1.0f) ? g : 0.0f;
}

// Why a (distortion, param, noise, H, W, input mode) tuple is refused, or nullptr after filling `d`.  For a mixed set everything any member could need is
// checked here, before a launch: which member a step uses is known on the device only.  lone_kinds: the kinds a single code may name at this entry point.
inline const char *describe_distortion(Distortion &d, uint32_t distortion, const float *param, const float *noise, uint32_t H, uint32_t W, uint32_t mode,
                                       uint32_t lone_kinds = kDistFusedKinds) {
    d = Distortion{kDistNone, H, W, nullptr, nullptr};
    const bool mixed = is_mixed(distortion);
    const uint32_t mask = kinds_mask(distortion);
    auto has = [mask](uint32_t kind) { return ((mask >> kind) & 1u) != 0; };
    if (!mixed && !(mask & lone_kinds)) return "the distortion code names no kind this entry point takes (rotation and scaling are wm_distort_geom_fwd / _bwd)";
    if (distortion == kDistNone) return nullptr;
    if (mode != 1) return mixed ? "the mixed distortion needs input_mode 1" : "a distortion needs input_mode 1";
    if (mixed && (mask == 0 || (mask & ~kDistAllKinds))) return "the mixed distortion's set is empty or holds bits beyond the kinds 0..5";
    if (param == nullptr && (mixed || !has(kDistNoise))) return mixed ? "the mixed distortion needs its parameter block (dist_param)" : "the kind needs its device parameter (dist_param)";
    if (has(kDistNoise) && noise == nullptr) return mixed ? "the mixed distortion's set holds noise: it needs the noise tensor (dist_noise)" : "noise needs the noise tensor (dist_noise)";
    if (has(kDistBlur) && (H < 2 || W < 2))      // reflect padding by one needs two pixels
        return mixed ? "the mixed distortion's set holds the blur: H and W must be at least 2" : "the blur needs H and W of at least 2";
    d.code = distortion & 0xFFFFu;      // (a mixed code's upper half, the block's image count, is the draw's alone)
    d.param = param;
    d.noise = noise;
    return nullptr;
}

// gx [B][H][W][C] = the layer's adjoint and the clamp's mask applied to gy (d.H, d.W: the image's): one launch whatever the kind (distortion.hip)
void launch_distort_adjoint(const float *gy, const float *img, const Distortion &d, uint32_t B, uint32_t C, float *gx, hipStream_t stream);

}  // namespace nsig
