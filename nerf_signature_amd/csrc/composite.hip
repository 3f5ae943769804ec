// Training compositing for gfx950: the front-to-back compositor over the marcher's sample rows (forward, backward, stage 1's one-launch form) and the render's
// elementwise tail (background mix, depth normalisation), stand-alone and folded into the compositing launches (raymarching.cu:501-693, renderer_wtmk.py:316-319).
//
// The entry points promise "the same bits as the separate launches" (the fused ones against rm_composite_train_fwd/_bwd, rm_finish_fwd/_bwd and clean_loss's seed).
// Built with -ffp-contract=off, the same operations in the same order give the same bits, so every piece of arithmetic here is ONE device function.
#include "wave.h"

namespace nsig {

// ----------------------------------------------------------------------------- the render tail of one ray (renderer_wtmk.py:316-319 / 369-372)

__device__ __forceinline__ float over_background(float c, float ws, float bg) { return c + (1.0f - ws) * bg; }

// NaN for rays that miss the box, as the reference
__device__ __forceinline__ float normalised_depth(float d, float near, float far) { return fmaxf(d - near, 0.0f) / (far - near); }

// image_out = image + (1 - weights_sum) * bg  =>  d weights_sum = -sum_c grad_image_out_c * bg_c
__device__ __forceinline__ float finish_adjoint(float g0, float g1, float g2, float bg0, float bg1, float bg2) {
    float s = 0.0f;
    s += g0 * bg0; s += g1 * bg1; s += g2 * bg2;
    return -s;
}

__global__ void __launch_bounds__(256) k_finish_fwd(const float *__restrict__ image, const float *__restrict__ depth, const float *__restrict__ ws,
                                                    const float *__restrict__ nears, const float *__restrict__ fars, const float *__restrict__ bg,
                                                    uint32_t bg_stride, uint32_t N, float *__restrict__ image_out, float *__restrict__ depth_out) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const float w = ws[i];
#pragma unroll
    for (int c = 0; c < 3; ++c) image_out[i * 3 + c] = over_background(image[i * 3 + c], w, bg[i * bg_stride + c]);
    depth_out[i] = normalised_depth(depth[i], nears[i], fars[i]);
}

__global__ void __launch_bounds__(256) k_finish_bwd(const float *__restrict__ g_image, const float *__restrict__ g_depth, const float *__restrict__ depth,
                                                    const float *__restrict__ nears, const float *__restrict__ fars, const float *__restrict__ bg,
                                                    uint32_t bg_stride, uint32_t N, float *__restrict__ g_ws, float *__restrict__ g_depth_in) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    float a = -0.0f;   // no grad_image: minus an empty sum
    if (g_image) a = finish_adjoint(g_image[i * 3], g_image[i * 3 + 1], g_image[i * 3 + 2], bg[i * bg_stride], bg[i * bg_stride + 1], bg[i * bg_stride + 2]);
    g_ws[i] = a;
    if (g_depth_in) g_depth_in[i] = (g_depth && depth[i] - nears[i] >= 0.0f) ? g_depth[i] / (fars[i] - nears[i]) : 0.0f;
}

// ----------------------------------------------------------------------------- the render tail as store bytes (rm_finish_u8; include/nerfsig.h pins the arithmetic)

__device__ __forceinline__ float unit_clamp(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }
__device__ __forceinline__ uint32_t unit_code(float x) { return (uint32_t)rintf(255.0f * unit_clamp(x)); }

struct Bg3 {
    float c[3];
};

// The pixel of ray i as a little-endian word: byte k in bits 8k .. 8k+7.  C = 4: straight (r, g, b) and alpha; C = 3: (r, g, b) over bg, the top byte 0.
template <int C> __device__ __forceinline__ uint32_t finish_code(const float *__restrict__ image, const float *__restrict__ ws, size_t i, const Bg3 &bg) {
    const float a = unit_clamp(ws[i]);
    uint32_t word = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float v = image[i * 3 + c];
        float x;
        if (C == 4) {
            x = a > 0.0f ? v / a : 0.0f;
        } else {
            const float behind = (1.0f - a) * bg.c[c];
            x = v + behind;
        }
        word |= unit_code(x) << (8 * c);
    }
    if (C == 4) word |= unit_code(a) << 24;      // (a is in [0, 1] already: rint(255 a))
    return word;
}

// One lane per ray, one 4-byte store per ray (byte stores when `out` is not 4-byte aligned: a uniform branch).
__global__ void __launch_bounds__(256) k_finish_u8_rgba(const float *__restrict__ image, const float *__restrict__ ws, uint32_t N, uint8_t *__restrict__ out,
                                                        uint32_t aligned) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const uint32_t word = finish_code<4>(image, ws, i, Bg3{});
    if (aligned) {
        reinterpret_cast<uint32_t *>(out)[i] = word;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) out[i * 4 + k] = (uint8_t)(word >> (8 * k));
    }
}

// Three bytes per ray.  A lane that owned one ray would issue a 2-byte and a 1-byte store, and a store costs its issue slot whatever its width (the row loads of
// DESIGN.md section 22 taught that for 4- / 2- / 1-byte words: the count binds, not the bytes) -- so a lane owns FOUR consecutive rays, 12 bytes = three aligned
// 4-byte stores, a quarter of the lanes and 3 stores per 4 rays instead of 8.  The rays before the first 4-byte boundary of `out` (head = address mod 4 of them:
// ray r starts at byte 3 r) and the (N - head) mod 4 rays behind the last whole group go to one lane each, behind the groups, with byte stores.
__global__ void __launch_bounds__(256) k_finish_u8_rgb(const float *__restrict__ image, const float *__restrict__ ws, uint32_t N, Bg3 bg, uint8_t *__restrict__ out,
                                                       uint32_t head, uint32_t groups) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;      // (groups + leftovers <= N: no wrap)
    if (t < groups) {
        const size_t r = (size_t)head + 4 * (size_t)t;
        const uint32_t w0 = finish_code<3>(image, ws, r, bg), w1 = finish_code<3>(image, ws, r + 1, bg);
        const uint32_t w2 = finish_code<3>(image, ws, r + 2, bg), w3 = finish_code<3>(image, ws, r + 3, bg);
        uint32_t *o = reinterpret_cast<uint32_t *>(out + 3 * r);
        o[0] = w0 | (w1 << 24);
        o[1] = (w1 >> 8) | (w2 << 16);
        o[2] = (w2 >> 16) | (w3 << 8);
        return;
    }
    const uint32_t k = t - groups;
    const size_t r = k < head ? (size_t)k : (size_t)head + 4 * (size_t)groups + (k - head);
    if (r >= N) return;
    const uint32_t word = finish_code<3>(image, ws, r, bg);
#pragma unroll
    for (int c = 0; c < 3; ++c) out[3 * r + c] = (uint8_t)(word >> (8 * c));
}

// ----------------------------------------------------------------------------- compositing (training)
//
// One wave per ray.  The reference walks a ray's samples serially (raymarching.cu:540-567); here the 64 lanes take 64
// consecutive samples (coalesced loads), the transmittance T_j = prod_{i<j} (1 - alpha_i) comes from a wave-level
// prefix product, the running depth parameter and (backward) the running colour from prefix sums, and the early
// exit `T < T_thresh` becomes a prefix mask: sample j is accumulated iff the transmittance after sample j-1 is still
// >= T_thresh (the reference tests after accumulating, :557).  Products and sums associate differently from the
// serial loop, so results agree to fp32 round-off, not bit for bit (they never could: the reference uses __expf).

struct Chunk {
    float alpha, w, T_after, c0, c1, c2, dt, dreal;
    bool valid, live;
};

// loads 64 samples of a ray and derives alpha, weight and transmittance; T_carry = transmittance entering the chunk
__device__ inline Chunk load_chunk(const float *__restrict__ sigmas, const float *__restrict__ rgbs, const float *__restrict__ deltas, size_t m0,
                                   uint32_t base, uint32_t cnt, int lane, float T_carry, float T_thresh) {
    Chunk c;
    c.valid = base + (uint32_t)lane < cnt;
    const size_t m = m0 + base + lane;
    float sigma = 0.0f;
    c.dt = c.dreal = c.c0 = c.c1 = c.c2 = 0.0f;
    if (c.valid) {
        sigma = sigmas[m];
        const float2 dl = reinterpret_cast<const float2 *>(deltas)[m];
        c.dt = dl.x; c.dreal = dl.y;
        c.c0 = rgbs[3 * m]; c.c1 = rgbs[3 * m + 1]; c.c2 = rgbs[3 * m + 2];
    }
    c.alpha = c.valid ? 1.0f - __expf(-sigma * c.dt) : 0.0f;
    const float P = wave_scan(1.0f - c.alpha, lane, [](float a, float b) { return a * b; });  // inclusive product
    float P_excl = __shfl_up(P, 1, 64);
    if (lane == 0) P_excl = 1.0f;
    const float T_before = T_carry * P_excl;
    c.T_after = T_carry * P;
    c.live = c.valid && T_before >= T_thresh;   // every earlier sample left T >= T_thresh (T_carry itself did)
    c.w = c.live ? c.alpha * T_before : 0.0f;
    return c;
}

// Optional tail of the render done by the ray's wave instead of a separate launch: background mix and depth normalisation in the forward, the
// weights_sum gradient of the background mix in the backward.
struct FinishArgs {
    const float *nears, *fars, *bg;   // bg == nullptr: no tail
    uint32_t bg_stride;               // 0: one colour [3]; 3: per ray
    float *image_out, *depth_out;     // forward outputs
    uint32_t self_zero;               // backward: the kernel zero-fills every gradient row it does not write (no memsets before it)
};

struct RaySums { float r, g, b, ws, d; };

// The forward walk over the chunks of a ray that fits (0 < cnt, off + cnt <= M): the wave's five sums, in every lane.
__device__ __forceinline__ RaySums composite_ray_fwd(const float *__restrict__ sigmas, const float *__restrict__ rgbs, const float *__restrict__ deltas,
                                                     uint32_t off, uint32_t cnt, int lane, float T_thresh) {
    float r = 0, g = 0, b = 0, ws = 0, d = 0, T = 1.0f, tt = 0.0f;
    for (uint32_t base = 0; base < cnt; base += 64) {
        const Chunk c = load_chunk(sigmas, rgbs, deltas, off, base, cnt, lane, T, T_thresh);
        const float t_incl = tt + wave_scan(c.dreal, lane, [](float a, float b2) { return a + b2; });  // accumulated real deltas (:549)
        r += c.w * c.c0; g += c.w * c.c1; b += c.w * c.c2; ws += c.w; d += c.w * t_incl;
        T = __shfl(c.T_after, 63, 64);
        tt = __shfl(t_incl, 63, 64);
        if (T < T_thresh) break;  // some sample of this chunk ended the ray
    }
    return RaySums{wave_sum(r), wave_sum(g), wave_sum(b), wave_sum(ws), wave_sum(d)};
}

__device__ __forceinline__ void zero_grad_row(size_t m, float *__restrict__ grad_sigmas, float *__restrict__ grad_rgbs) {
    grad_sigmas[m] = 0.0f;
    grad_rgbs[3 * m] = 0.0f; grad_rgbs[3 * m + 1] = 0.0f; grad_rgbs[3 * m + 2] = 0.0f;
}

// [first, last) of the range of the ray at `off`, clipped to M, by the ray's wave.  A closure over the caller's variables and deliberately not
// __forceinline__: inlined early, the compiler rewrites the loop's bounds, and the self-zeroing backward came out 5 % slower at the block render's shape
// (LABNOTES, "Compositing in one source").  Inlined late it compiles to the instructions of the lambda it replaces.
struct ZeroRayRows {
    const uint32_t &off, &M; const int &lane;
    float *__restrict__ const &grad_sigmas, *__restrict__ const &grad_rgbs;
    __device__ void operator()(uint32_t first, uint32_t last) const {
        for (size_t m = (size_t)off + first + lane; m < (size_t)off + last && m < M; m += 64) zero_grad_row(m, grad_sigmas, grad_rgbs);
    }
};

// The workgroups behind the ceil_div(N, 4) that own rays: rows past the last ray's samples (padding / unused capacity).  Rays are in ascending, gapless offset order.
__device__ __forceinline__ void zero_tail_rows(const int32_t *__restrict__ rays, uint32_t M, uint32_t N, float *__restrict__ grad_sigmas, float *__restrict__ grad_rgbs) {
    const uint32_t total = (uint32_t)rays[3 * (size_t)(N - 1) + 1] + (uint32_t)rays[3 * (size_t)(N - 1) + 2];
    for (size_t m = (size_t)total + (size_t)(blockIdx.x - ceil_div(N, 4u)) * 256 + threadIdx.x; m < M; m += (size_t)(gridDim.x - ceil_div(N, 4u)) * 256)
        zero_grad_row(m, grad_sigmas, grad_rgbs);
}

// The backward walk over the chunks of a ray that fits (raymarching.cu:602-682; grad_depth does not propagate, raymarching.py:275).  (g0, g1, g2) = the
// gradient of the ray's image, (rf, gf, bf) = the image itself, tail = grad_weights_sum * (1 - weights_sum).  Only live samples are written; with
// self_zero the wave also zero-fills the ray's other rows: dead samples of a chunk and everything behind the chunk that ended the ray.
__device__ __forceinline__ void composite_ray_bwd(const float *__restrict__ sigmas, const float *__restrict__ rgbs, const float *__restrict__ deltas, uint32_t off,
                                                  uint32_t cnt, uint32_t M, int lane, float T_thresh, float g0, float g1, float g2, float rf, float gf, float bf,
                                                  float tail, bool self_zero, float *__restrict__ grad_sigmas, float *__restrict__ grad_rgbs) {
    const ZeroRayRows zero_rows{off, M, lane, grad_sigmas, grad_rgbs};
    float T = 1.0f, r = 0.0f, g = 0.0f, b = 0.0f;  // carries: transmittance and accumulated colour entering the chunk
    auto add = [](float a, float c) { return a + c; };
    for (uint32_t base = 0; base < cnt; base += 64) {
        const Chunk c = load_chunk(sigmas, rgbs, deltas, off, base, cnt, lane, T, T_thresh);
        const float r_incl = r + wave_scan(c.w * c.c0, lane, add);
        const float g_incl = g + wave_scan(c.w * c.c1, lane, add);
        const float b_incl = b + wave_scan(c.w * c.c2, lane, add);
        if (c.live) {
            const size_t m = (size_t)off + base + lane;
            grad_rgbs[3 * m] = g0 * c.w; grad_rgbs[3 * m + 1] = g1 * c.w; grad_rgbs[3 * m + 2] = g2 * c.w;
            grad_sigmas[m] = c.dt * (g0 * (c.T_after * c.c0 - (rf - r_incl)) + g1 * (c.T_after * c.c1 - (gf - g_incl)) +
                                     g2 * (c.T_after * c.c2 - (bf - b_incl)) + tail);
        } else if (self_zero && base + lane < cnt) {
            zero_grad_row((size_t)off + base + lane, grad_sigmas, grad_rgbs);
        }
        T = __shfl(c.T_after, 63, 64);
        r = __shfl(r_incl, 63, 64); g = __shfl(g_incl, 63, 64); b = __shfl(b_incl, 63, 64);
        if (T < T_thresh) {   // the ray ended in this chunk: later samples get no gradient
            if (self_zero) zero_rows(base + 64, cnt);
            break;
        }
    }
}

__global__ void __launch_bounds__(256) k_composite_fwd(const float *__restrict__ sigmas, const float *__restrict__ rgbs, const float *__restrict__ deltas,
                                                       const int32_t *__restrict__ rays, uint32_t M, uint32_t N, float T_thresh, float *__restrict__ weights_sum,
                                                       float *__restrict__ depth, float *__restrict__ image, FinishArgs fin = FinishArgs{}) {
    const int lane = threadIdx.x & 63;
    const uint32_t n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    const uint32_t id = (uint32_t)rays[3 * (size_t)n], off = (uint32_t)rays[3 * (size_t)n + 1], cnt = (uint32_t)rays[3 * (size_t)n + 2];
    RaySums s{0, 0, 0, 0, 0};
    if (cnt != 0 && off + cnt <= M) s = composite_ray_fwd(sigmas, rgbs, deltas, off, cnt, lane, T_thresh);
    if (lane == 0) {
        weights_sum[id] = s.ws;
        depth[id] = s.d;
        image[3 * (size_t)id] = s.r; image[3 * (size_t)id + 1] = s.g; image[3 * (size_t)id + 2] = s.b;
        if (fin.bg != nullptr) {
            const float *bgp = fin.bg + (size_t)id * fin.bg_stride;
            fin.image_out[3 * (size_t)id] = over_background(s.r, s.ws, bgp[0]);
            fin.image_out[3 * (size_t)id + 1] = over_background(s.g, s.ws, bgp[1]);
            fin.image_out[3 * (size_t)id + 2] = over_background(s.b, s.ws, bgp[2]);
            fin.depth_out[id] = normalised_depth(s.d, fin.nears[id], fin.fars[id]);
        }
    }
}

// Without fin.self_zero the grad buffers are pre-zeroed by the host wrapper.
__global__ void __launch_bounds__(256) k_composite_bwd(const float *__restrict__ grad_ws, const float *__restrict__ grad_image, const float *__restrict__ sigmas,
                                                       const float *__restrict__ rgbs, const float *__restrict__ deltas, const int32_t *__restrict__ rays,
                                                       const float *__restrict__ weights_sum, const float *__restrict__ image, uint32_t M, uint32_t N,
                                                       float T_thresh, float *__restrict__ grad_sigmas, float *__restrict__ grad_rgbs, FinishArgs fin = FinishArgs{}) {
    const int lane = threadIdx.x & 63;
    if (fin.self_zero && blockIdx.x >= ceil_div(N, 4u)) { zero_tail_rows(rays, M, N, grad_sigmas, grad_rgbs); return; }
    const uint32_t n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    const uint32_t id = (uint32_t)rays[3 * (size_t)n], off = (uint32_t)rays[3 * (size_t)n + 1], cnt = (uint32_t)rays[3 * (size_t)n + 2];
    if (cnt == 0) return;
    if (off + cnt > M) {   // a ray that did not fit (bounded mode): no gradient, but its rows below M belong to nobody else
        if (fin.self_zero) ZeroRayRows{off, M, lane, grad_sigmas, grad_rgbs}(0, cnt);
        return;
    }
    const float g0 = grad_image[3 * (size_t)id], g1 = grad_image[3 * (size_t)id + 1], g2 = grad_image[3 * (size_t)id + 2];
    const float rf = image[3 * (size_t)id], gf = image[3 * (size_t)id + 1], bf = image[3 * (size_t)id + 2];
    float gws = grad_ws != nullptr ? grad_ws[id] : 0.0f;
    if (fin.bg != nullptr) {
        const float *bgp = fin.bg + (size_t)id * fin.bg_stride;
        gws = gws + finish_adjoint(g0, g1, g2, bgp[0], bgp[1], bgp[2]);
    }
    composite_ray_bwd(sigmas, rgbs, deltas, off, cnt, M, lane, T_thresh, g0, g1, g2, rf, gf, bf, gws * (1.0f - weights_sum[id]), fin.self_zero != 0,
                      grad_sigmas, grad_rgbs);
}

// Stage 1's compositing in ONE launch (stage1.GraphedCleanLoop): k_composite_fwd with the render tail, the gradient half of k_clean_loss
// (nerf/utils.py:503: d loss / d image = grad_k * (image - gt), grad_k = mse_seed_factor(grad_scale, n_values)) and k_composite_bwd with the tail's adjoint
// and self_zero, for rays in ascending gapless offset order.  A wave owns a ray in all three, so the ray's image never leaves its registers: forward over the
// ray's chunks, the three seed values, backward over the same chunks (read again, from L2).  The loss VALUE and the loop's books stay with clean_loss, launched
// behind this kernel: two launches in a row where there were three.
__global__ void __launch_bounds__(256) k_composite_mse(const float *__restrict__ sigmas, const float *__restrict__ rgbs, const float *__restrict__ deltas,
                                                       const int32_t *__restrict__ rays, uint32_t M, uint32_t N, float T_thresh, const float *__restrict__ gt,
                                                       float grad_k, FinishArgs fin, float *__restrict__ weights_sum, float *__restrict__ depth,
                                                       float *__restrict__ image, float *__restrict__ grad_image, float *__restrict__ grad_sigmas,
                                                       float *__restrict__ grad_rgbs) {
    const int lane = threadIdx.x & 63;
    if (blockIdx.x >= ceil_div(N, 4u)) { zero_tail_rows(rays, M, N, grad_sigmas, grad_rgbs); return; }
    const uint32_t n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    const uint32_t id = (uint32_t)rays[3 * (size_t)n], off = (uint32_t)rays[3 * (size_t)n + 1], cnt = (uint32_t)rays[3 * (size_t)n + 2];
    const bool fits = cnt != 0 && off + cnt <= M;
    RaySums s{0, 0, 0, 0, 0};
    if (fits) s = composite_ray_fwd(sigmas, rgbs, deltas, off, cnt, lane, T_thresh);
    const float *bgp = fin.bg + (size_t)id * fin.bg_stride;
    const float bg0 = bgp[0], bg1 = bgp[1], bg2 = bgp[2];
    const float o0 = over_background(s.r, s.ws, bg0), o1 = over_background(s.g, s.ws, bg1), o2 = over_background(s.b, s.ws, bg2);
    const float g0 = grad_k * (o0 - gt[3 * (size_t)id]), g1 = grad_k * (o1 - gt[3 * (size_t)id + 1]), g2 = grad_k * (o2 - gt[3 * (size_t)id + 2]);   // k_clean_loss's seed
    if (lane == 0) {
        weights_sum[id] = s.ws;
        depth[id] = s.d;
        image[3 * (size_t)id] = s.r; image[3 * (size_t)id + 1] = s.g; image[3 * (size_t)id + 2] = s.b;
        fin.image_out[3 * (size_t)id] = o0; fin.image_out[3 * (size_t)id + 1] = o1; fin.image_out[3 * (size_t)id + 2] = o2;
        fin.depth_out[id] = normalised_depth(s.d, fin.nears[id], fin.fars[id]);
        grad_image[3 * (size_t)id] = g0; grad_image[3 * (size_t)id + 1] = g1; grad_image[3 * (size_t)id + 2] = g2;
    }
    if (cnt == 0) return;
    if (!fits) { ZeroRayRows{off, M, lane, grad_sigmas, grad_rgbs}(0, cnt); return; }
    const float gws = 0.0f + finish_adjoint(g0, g1, g2, bg0, bg1, bg2);   // k_composite_bwd with a null grad_ws
    composite_ray_bwd(sigmas, rgbs, deltas, off, cnt, M, lane, T_thresh, g0, g1, g2, s.r, s.g, s.b, gws * (1.0f - s.ws), true, grad_sigmas, grad_rgbs);
}

}  // namespace nsig

// ============================================================================= C ABI

using namespace nsig;

static int zero_gradients(const char *who, float *grad_sigmas, float *grad_rgbs, uint32_t M, nsig_stream_t stream) {
    if (hipMemsetAsync(grad_sigmas, 0, (size_t)M * sizeof(float), as_stream(stream)) != hipSuccess ||
        hipMemsetAsync(grad_rgbs, 0, (size_t)M * 3 * sizeof(float), as_stream(stream)) != hipSuccess) {
        set_error("%s: hipMemsetAsync failed", who);
        return NSIG_ERR_LAUNCH;
    }
    return NSIG_OK;   // both gradient buffers zeroed
}

NSIG_EXPORT int rm_composite_train_fwd(const float *sigmas, const float *rgbs, const float *deltas,
                                       const int32_t *rays, uint32_t M, uint32_t N, float T_thresh, float *weights_sum,
                                       float *depth, float *image, nsig_stream_t stream) {
    if (N == 0) return NSIG_OK;
    NSIG_REQUIRE(sigmas && rgbs && deltas && rays && weights_sum && depth && image, "rm_composite_train_fwd: null pointer");
    k_composite_fwd<<<ceil_div(N, 4u), 256, 0, as_stream(stream)>>>(sigmas, rgbs, deltas, rays, M, N, T_thresh, weights_sum, depth, image);
    return check_launch("rm_composite_train_fwd");
}

NSIG_EXPORT int rm_composite_train_bwd(const float *grad_weights_sum, const float *grad_image, const float *sigmas,
                                       const float *rgbs, const float *deltas, const int32_t *rays,
                                       const float *weights_sum, const float *image, uint32_t M, uint32_t N,
                                       float T_thresh, float *grad_sigmas, float *grad_rgbs, nsig_stream_t stream) {
    if (M == 0) return NSIG_OK;
    NSIG_REQUIRE(grad_weights_sum && grad_image && sigmas && rgbs && deltas && rays && weights_sum && image && grad_sigmas && grad_rgbs,
                 "rm_composite_train_bwd: null pointer");
    if (int e = zero_gradients("rm_composite_train_bwd", grad_sigmas, grad_rgbs, M, stream)) return e;
    if (N == 0) return NSIG_OK;
    k_composite_bwd<<<ceil_div(N, 4u), 256, 0, as_stream(stream)>>>(grad_weights_sum, grad_image, sigmas, rgbs, deltas, rays,
                                                                        weights_sum, image, M, N, T_thresh, grad_sigmas, grad_rgbs);
    return check_launch("rm_composite_train_bwd");
}

NSIG_EXPORT int rm_composite_train_finish_fwd(const float *sigmas, const float *rgbs, const float *deltas, const int32_t *rays, uint32_t M,
                                              uint32_t N, float T_thresh, const float *nears, const float *fars, const float *bg,
                                              uint32_t bg_stride, float *weights_sum, float *depth, float *image, float *image_out,
                                              float *depth_out, nsig_stream_t stream) {
    if (N == 0) return NSIG_OK;
    NSIG_REQUIRE(sigmas && rgbs && deltas && rays && weights_sum && depth && image && nears && fars && bg && image_out && depth_out,
                 "rm_composite_train_finish_fwd: null pointer");
    NSIG_REQUIRE(bg_stride == 0 || bg_stride == 3, "rm_composite_train_finish_fwd: bg_stride is 0 (one colour) or 3 (per ray)");
    const FinishArgs fin{nears, fars, bg, bg_stride, image_out, depth_out, 0u};
    k_composite_fwd<<<ceil_div(N, 4u), 256, 0, as_stream(stream)>>>(sigmas, rgbs, deltas, rays, M, N, T_thresh, weights_sum, depth, image, fin);
    return check_launch("rm_composite_train_finish_fwd");
}

NSIG_EXPORT int rm_composite_train_finish_bwd(const float *grad_weights_sum, const float *grad_image_out, const float *sigmas, const float *rgbs,
                                              const float *deltas, const int32_t *rays, const float *weights_sum, const float *image,
                                              const float *bg, uint32_t bg_stride, uint32_t M, uint32_t N, float T_thresh, uint32_t rays_in_order,
                                              float *grad_sigmas, float *grad_rgbs, nsig_stream_t stream) {
    if (M == 0) return NSIG_OK;
    NSIG_REQUIRE(grad_image_out && sigmas && rgbs && deltas && rays && weights_sum && image && bg && grad_sigmas && grad_rgbs,
                 "rm_composite_train_finish_bwd: null pointer");
    NSIG_REQUIRE(bg_stride == 0 || bg_stride == 3, "rm_composite_train_finish_bwd: bg_stride is 0 (one colour) or 3 (per ray)");
    const bool self_zero = rays_in_order != 0 && N != 0;
    if (!self_zero)
        if (int e = zero_gradients("rm_composite_train_finish_bwd", grad_sigmas, grad_rgbs, M, stream)) return e;
    if (N == 0) return NSIG_OK;
    const FinishArgs fin{nullptr, nullptr, bg, bg_stride, nullptr, nullptr, self_zero ? 1u : 0u};
    k_composite_bwd<<<ceil_div(N, 4u) + (self_zero ? 64u : 0u), 256, 0, as_stream(stream)>>>(grad_weights_sum, grad_image_out, sigmas, rgbs, deltas, rays, weights_sum, image, M, N,
                                                                    T_thresh, grad_sigmas, grad_rgbs, fin);
    return check_launch("rm_composite_train_finish_bwd");
}

NSIG_EXPORT int rm_composite_train_mse(const float *sigmas, const float *rgbs, const float *deltas, const int32_t *rays, uint32_t M, uint32_t N, float T_thresh,
                                       const float *nears, const float *fars, const float *bg, uint32_t bg_stride, const float *gt, uint32_t n_values,
                                       float grad_scale, float *weights_sum, float *depth, float *image, float *image_out, float *depth_out, float *grad_image,
                                       float *grad_sigmas, float *grad_rgbs, nsig_stream_t stream) {
    if (N == 0) return NSIG_OK;
    NSIG_REQUIRE(sigmas && rgbs && deltas && rays && nears && fars && bg && gt && weights_sum && depth && image && image_out && depth_out && grad_image &&
                 grad_sigmas && grad_rgbs, "rm_composite_train_mse: null pointer");
    NSIG_REQUIRE(bg_stride == 0 || bg_stride == 3, "rm_composite_train_mse: bg_stride is 0 (one colour) or 3 (per ray)");
    NSIG_REQUIRE(n_values >= 1, "rm_composite_train_mse: n_values must be positive");
    const FinishArgs fin{nears, fars, bg, bg_stride, image_out, depth_out, 1u};
    k_composite_mse<<<ceil_div(N, 4u) + 64u, 256, 0, as_stream(stream)>>>(sigmas, rgbs, deltas, rays, M, N, T_thresh, gt, mse_seed_factor(grad_scale, n_values), fin,
                                                                         weights_sum, depth, image, grad_image, grad_sigmas, grad_rgbs);
    return check_launch("rm_composite_train_mse");
}

NSIG_EXPORT int rm_finish_fwd(const float *image, const float *depth, const float *weights_sum, const float *nears, const float *fars,
                              const float *bg, uint32_t bg_stride, uint32_t N, float *image_out, float *depth_out, nsig_stream_t stream) {
    if (N == 0) return NSIG_OK;
    NSIG_REQUIRE(image && depth && weights_sum && nears && fars && bg && image_out && depth_out, "rm_finish_fwd: null pointer");
    NSIG_REQUIRE(bg_stride == 0 || bg_stride == 3, "rm_finish_fwd: bg_stride is 0 (one colour) or 3 (per ray)");
    k_finish_fwd<<<ceil_div(N, 256u), 256, 0, as_stream(stream)>>>(image, depth, weights_sum, nears, fars, bg, bg_stride, N, image_out, depth_out);
    return check_launch("rm_finish_fwd");
}

NSIG_EXPORT int rm_finish_u8(const float *image, const float *weights_sum, uint32_t N, uint32_t channels, float bg_r, float bg_g, float bg_b, uint8_t *out,
                             nsig_stream_t stream) {
    NSIG_REQUIRE(channels == 3 || channels == 4, "rm_finish_u8: channels=%u is not 3 or 4", channels);
    if (N == 0) return NSIG_OK;
    NSIG_REQUIRE(image && weights_sum && out, "rm_finish_u8: null pointer");
    const uint32_t phase = (uint32_t)(reinterpret_cast<uintptr_t>(out) & 3u);
    if (channels == 4) {
        k_finish_u8_rgba<<<(uint32_t)(((uint64_t)N + 255u) / 256u), 256, 0, as_stream(stream)>>>(image, weights_sum, N, out, phase == 0u ? 1u : 0u);
    } else {
        const uint32_t head = phase < N ? phase : N;
        const uint32_t groups = (N - head) / 4u;
        const uint32_t lanes = groups + (N - 4u * groups);      // one per group, one per ray outside the groups (at most 6)
        k_finish_u8_rgb<<<(uint32_t)(((uint64_t)lanes + 255u) / 256u), 256, 0, as_stream(stream)>>>(image, weights_sum, N, Bg3{{bg_r, bg_g, bg_b}}, out, head, groups);
    }
    return check_launch("rm_finish_u8");
}

NSIG_EXPORT int rm_finish_bwd(const float *grad_image, const float *grad_depth, const float *depth, const float *nears, const float *fars,
                              const float *bg, uint32_t bg_stride, uint32_t N, float *grad_weights_sum, float *grad_depth_in, nsig_stream_t stream) {
    if (N == 0) return NSIG_OK;
    NSIG_REQUIRE(depth && nears && fars && bg && grad_weights_sum, "rm_finish_bwd: null pointer");
    NSIG_REQUIRE(bg_stride == 0 || bg_stride == 3, "rm_finish_bwd: bg_stride is 0 (one colour) or 3 (per ray)");
    k_finish_bwd<<<ceil_div(N, 256u), 256, 0, as_stream(stream)>>>(grad_image, grad_depth, depth, nears, fars, bg, bg_stride, N, grad_weights_sum, grad_depth_in);
    return check_launch("rm_finish_bwd");
}
