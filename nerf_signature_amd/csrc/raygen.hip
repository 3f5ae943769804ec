// Ray generation for gfx950 (include/nerfsig.h, "ray generation"): the rays of given pixels (rg_get_rays), and one training batch straight from a device-resident
// store -- pixel indices drawn uniformly, by the error map's race, or for a drawn orbit camera; float32 or uint8 pixels, RGB or RGBA with a random background --
// plus the error map's update.  One launch each, no host value in it: they sit inside a captured training step.  Nothing here marches (csrc/raymarch.hip).
// The draws are draws.h's 32-bit family (streams 0..5 of a step), the ray arithmetic is rays.h's pixel_ray.  Built with -ffp-contract=off: every product and sum
// below is rounded on its own, which the bit-exact host mirrors rely on (tests/error_map_ref.py, random_bg_ref.py, orbit_ref.py).
#include "draws.h"
#include "rays.h"
#include "wave.h"
#include <float.h>

namespace nsig {

// get_rays (nerf/utils_wtmk_disen.py:121-141) for given pixel indices: one lane per ray, no [B, H*W] meshgrid.
__global__ void k_get_rays(const float *__restrict__ poses, float fx, float fy, float cx, float cy, uint32_t H, uint32_t W,
                           const int64_t *__restrict__ inds, uint32_t B, uint32_t N, float *__restrict__ rays_o,
                           float *__restrict__ rays_d) {
    const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= B * N) return;
    const uint32_t b = gid / N, n = gid % N;
    const int64_t ind = inds ? inds[(size_t)b * N + n] : (int64_t)n;
    const float i = (float)(ind % (int64_t)W) + 0.5f, j = (float)(ind / (int64_t)W) + 0.5f;  // pixel centres (:76-77)
    pixel_ray(poses + 16 * (size_t)b, fx, fy, cx, cy, i, j, rays_o + 3 * (size_t)gid, rays_d + 3 * (size_t)gid);
}

// The stage-1 step on RGBA ground truth (nerf/utils.py:498-507): a fresh background colour per pixel, bg = torch.rand_like(images[..., :3]), and the target
// gt = rgb * a + bg * (1 - a).  bg[c] of ray n is word 3 n + c of sequence 4 of the step's counter hash, on torch.rand's grid (24 bits * 2^-24, exact in fp32);
// the blend in the reference's operation order with every product and sum rounded on its own (the file is built without contraction; the intrinsics say so
// where it matters), so that it equals the torch expression on the same operands bit for bit.  The one place the blend is written: the stand-alone kernel and
// both RGBA samplers call it.
__device__ inline void blend_random_background(float4 px, uint32_t bg_base, uint32_t n, float *__restrict__ bg_out, float *__restrict__ gt) {
    const float rgb[3] = {px.x, px.y, px.z};
    const float rest = __fsub_rn(1.0f, px.w);
#pragma unroll
    for (uint32_t c = 0; c < 3u; ++c) {
        const float b = unit24(draw_word(bg_base, 3u * n + c) >> 8);
        bg_out[3 * (size_t)n + c] = b;
        if (gt != nullptr) gt[3 * (size_t)n + c] = __fadd_rn(__fmul_rn(rgb[c], px.w), __fmul_rn(b, rest));
    }
}

__global__ void k_blend_random_background(const float4 *__restrict__ rgba, uint32_t N, const int32_t *__restrict__ step_counter, uint32_t seed_lo, uint32_t seed_hi,
                                          float *__restrict__ bg_out, float *__restrict__ gt_out) {
    const uint32_t n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const uint32_t step = step_counter ? (uint32_t)step_counter[0] : 0u;
    blend_random_background(rgba[n], draw_base(seed_lo, seed_hi, step, kBackgroundStream), n, bg_out, gt_out);
}

// The image store a sampler draws from, as the pixel fetch of write_sampled_ray: float32 pixels as they are stored, or uint8 codes decoded on the fetch
// (the reference decodes a whole dataset up front, nerf/provider.py:221 image.astype(np.float32) / 255: the same IEEE division, here on the drawn pixels only,
// so a sampler over a u8 store writes the bits of the float sampler over store.float() / 255).  pixel < P * H * W: no fetch leaves [px, px + P*H*W*channels).
struct FloatStore {
    static constexpr uint32_t kRgbaAlign = 16;                    // one 16-byte load per RGBA pixel
    const float *__restrict__ px;
    __device__ float4 rgba(size_t pixel) const { return reinterpret_cast<const float4 *>(px)[pixel]; }
    __device__ void rgb(size_t pixel, float (&c)[3]) const { c[0] = px[3 * pixel]; c[1] = px[3 * pixel + 1]; c[2] = px[3 * pixel + 2]; }
};
struct U8Store {
    static constexpr uint32_t kRgbaAlign = 4;                     // one 4-byte load per RGBA pixel
    const uint8_t *__restrict__ px;
    const float *__restrict__ decode;                             // float[256] for the colour codes (a colour-space table), or NULL: q / 255
    __device__ static float unit(uint32_t q) { return __fdiv_rn((float)q, 255.0f); }           // (q * (1/255) has other bits for 126 of the 256 codes)
    // the three colour codes of a pixel at once: one uniform branch, the table's three loads (or the three divisions) side by side
    __device__ void colours(uint32_t q0, uint32_t q1, uint32_t q2, float (&c)[3]) const {
        if (decode != nullptr) { c[0] = decode[q0]; c[1] = decode[q1]; c[2] = decode[q2]; }
        else { c[0] = unit(q0); c[1] = unit(q1); c[2] = unit(q2); }
    }
    __device__ float4 rgba(size_t pixel) const {
        const uint32_t w = reinterpret_cast<const uint32_t *>(px)[pixel];
        float c[3];
        colours(w & 255u, (w >> 8) & 255u, (w >> 16) & 255u, c);
        return make_float4(c[0], c[1], c[2], unit(w >> 24));
    }
    // three byte loads at any of the four byte phases of 3 * pixel, issued together: the words around a pixel reach past both ends of the store (its first and its
    // last pixel), and the launch is bound by its latency, not by its loads (tools/store_bench.py)
    __device__ void rgb(size_t pixel, float (&c)[3]) const {
        const uint8_t *b = px + 3 * pixel;
        const uint32_t q0 = b[0], q1 = b[1], q2 = b[2];
        colours(q0, q1, q2, c);
    }
};

// One training batch straight from a device-resident store of poses and images (the loader step in front of the
// path, nerf/provider_wtmk.py:585-600 + get_rays with N > 0, nerf/utils_wtmk_disen.py:103-106,121-141): pose p = (step * stride +
// offset) mod P with `step` read from a device counter, N pixel indices drawn uniformly from a counter-based hash of (seed, step, ray)
// (the reference draws torch.randint on its device: same distribution, another generator), their rays, and the pixels' colours of
// image p as ground truth.  One launch, no host value in it: it sits inside a captured training step.
// SampleBatch is what every sampler launch is handed, by value: the pose store, the camera, the step's counter and seed, and where the batch goes.  The image
// store travels beside it (its type is the kernels' template argument); the orbit sampler has no pose store (poses == nullptr, P == 0) and writes no ground truth.
struct SampleBatch {
    const float *__restrict__ poses;      // [P][4][4] camera-to-world, row-major
    uint32_t P;
    float fx, fy, cx, cy;
    uint32_t H, W, N;
    const int32_t *__restrict__ step_counter;      // the device's step count; nullptr: step 0
    uint32_t stride, offset, seed_lo, seed_hi;
    float *__restrict__ rays_o, *__restrict__ rays_d, *__restrict__ gt;      // [N][3] each; gt optional
    int64_t *__restrict__ inds_out;       // [N] pixel indices, optional
    int32_t *__restrict__ pose_out;       // [1] the step's pose index, optional
    float *__restrict__ bg_out;           // [N][3] RGBA only: the background colours drawn
    __device__ uint32_t step() const { return step_counter ? (uint32_t)step_counter[0] : 0u; }
    __device__ uint32_t pose_of(uint32_t step) const { return (uint32_t)(((uint64_t)step * stride + offset) % P); }
    __device__ uint32_t base(uint32_t step, uint32_t stream) const { return draw_base(seed_lo, seed_hi, step, stream); }
    // ray n's pixel of a uniform draw: word n of the pixel stream scaled to [0, H*W) by the high half of a 64-bit product
    __device__ uint32_t uniform_pixel(uint32_t step, uint32_t n) const { return (uint32_t)(((uint64_t)draw_word(base(step, kPixelStream), n) * ((uint64_t)H * W)) >> 32); }
};

// Ray n of a drawn batch: pixel `ind` of pose p -- the ray arithmetic of k_get_rays, the stored pixel as ground truth.  Shared by both store samplers.
// RGBA: the store holds [P, H*W, 4] (one load per pixel); the ray's background colour goes to bg_out and the ground truth is the blend against it.
template <bool RGBA, class Store>
__device__ inline void write_sampled_ray(const SampleBatch &b, Store store, uint32_t p, uint32_t ind, uint32_t n, uint32_t bg_base) {
    const float i = (float)(ind % b.W) + 0.5f, j = (float)(ind / b.W) + 0.5f;                  // as k_get_rays
    pixel_ray(b.poses + 16 * (size_t)p, b.fx, b.fy, b.cx, b.cy, i, j, b.rays_o + 3 * (size_t)n, b.rays_d + 3 * (size_t)n);
    if constexpr (RGBA) {
        blend_random_background(store.rgba((size_t)p * b.H * b.W + ind), bg_base, n, b.bg_out, b.gt);
    } else if (b.gt != nullptr) {
        float c[3];
        store.rgb((size_t)p * b.H * b.W + ind, c);
        b.gt[3 * (size_t)n] = c[0]; b.gt[3 * (size_t)n + 1] = c[1]; b.gt[3 * (size_t)n + 2] = c[2];
    }
    if (b.inds_out != nullptr) b.inds_out[n] = (int64_t)ind;
}

template <bool RGBA, class Store>
__global__ void k_sample_rays(SampleBatch b, Store store) {
    const uint32_t n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= b.N) return;
    const uint32_t step = b.step(), p = b.pose_of(step);
    write_sampled_ray<RGBA>(b, store, p, b.uniform_pixel(step, n), n, RGBA ? b.base(step, kBackgroundStream) : 0u);
    if (b.pose_out != nullptr && n == 0) b.pose_out[0] = (int32_t)p;
}

// rg_sample_rays without a store: the step's camera is drawn, not looked up.  One orbit pose looking at the origin -- the closed form blocks.rand_poses documents
// (the reference's rand_poses, nerf/provider_wtmk.py:60-96: polar angle first) -- from the two first words of sequence 5 of the counter hash of
// (seed, k = step * stride + offset), on torch.rand's 24-bit grid; products in rand_poses' order, every one rounded on its own.  Every lane derives the same pose
// (the same instructions on the same words: the same bits); lane 0 of the launch writes it out.
struct OrbitRange { float radius, theta0, theta1, phi0, phi1; };
__device__ inline void orbit_pose(uint32_t base, const OrbitRange &r, float (&Pm)[16]) {
    const float u_t = unit24(draw_word(base, 0u) >> 8), u_p = unit24(draw_word(base, 1u) >> 8);
    const float theta = __fadd_rn(__fmul_rn(u_t, __fsub_rn(r.theta1, r.theta0)), r.theta0);      // torch.rand(size) * (hi - lo) + lo
    const float phi = __fadd_rn(__fmul_rn(u_p, __fsub_rn(r.phi1, r.phi0)), r.phi0);
    const float st = sinf(theta), ct = cosf(theta), sp = sinf(phi), cp = cosf(phi);
    const float rs = __fmul_rn(r.radius, st);
    Pm[0] = -cp;   Pm[1] = __fmul_rn(ct, sp);   Pm[2] = -__fmul_rn(st, sp);   Pm[3] = __fmul_rn(rs, sp);
    Pm[4] = 0.0f;  Pm[5] = -st;                 Pm[6] = -ct;                  Pm[7] = __fmul_rn(r.radius, ct);
    Pm[8] = sp;    Pm[9] = __fmul_rn(ct, cp);   Pm[10] = -__fmul_rn(st, cp);  Pm[11] = __fmul_rn(rs, cp);
    Pm[12] = 0.0f; Pm[13] = 0.0f;               Pm[14] = 0.0f;                Pm[15] = 1.0f;
}

__global__ void k_sample_rays_orbit(SampleBatch b, OrbitRange range, float *__restrict__ pose_out) {
    const uint32_t n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= b.N) return;
    const uint32_t step = b.step();
    float Pm[16];
    orbit_pose(b.base(step * b.stride + b.offset, kOrbitStream), range, Pm);
    const uint32_t ind = b.uniform_pixel(step, n);
    const float i = (float)(ind % b.W) + 0.5f, j = (float)(ind / b.W) + 0.5f;                  // as k_get_rays
    pixel_ray(Pm, b.fx, b.fy, b.cx, b.cy, i, j, b.rays_o + 3 * (size_t)n, b.rays_d + 3 * (size_t)n);
    if (b.inds_out != nullptr) b.inds_out[n] = (int64_t)ind;
    if (n == 0) {
#pragma unroll
        for (int e = 0; e < 16; ++e) pose_out[e] = Pm[e];
    }
}

// The same batch drawn from pose p's error map (the reference's --error_map loader: nerf/utils.py:105-114 draws N of the map's G x G cells with
// torch.multinomial(replacement=False), then a uniform pixel inside each cell).  multinomial without replacement is an exponential race -- key = w / Exp(1),
// take the N largest -- and so is this: key(c) = w_c / -ln(u_c), u_c in (0, 1] from the counter hash of (seed, step, c).  The same distribution from another
// generator, which is the stance k_sample_rays takes.  A weight that is not finite or not positive has key 0 and is drawn only when fewer than N cells are
// valid (torch raises there; a captured step must not fault: the lowest-index invalid cells fill up).
//
// ONE workgroup of 1024 threads owns the draw; every thread keeps its (up to 16) keys in registers for the whole launch.  Cell c sits with wave c / (64 R),
// register (c / 64) % R, lane c % 64 (R = ceil(G*G / 1024) registers per lane), so ascending c is (wave, register, lane) order and a wave's ballots rank its cells.
//   select : non-negative floats order as their bit patterns -- radix select over the 32 key bits, 8 bits a pass, most significant first: the keys that
//            still match the threshold's known prefix are counted into an LDS histogram (kHistCopies copies, one per lane mod 32: an all-ones map puts
//            every key of a pass into one or two bins), a wave scans the 256 bins from the top -> threshold key T and the number of keys above it;
//   compact: every key > T is drawn, and the first N - above keys == T in cell order (equal keys go to the lower cell); ballots rank the cells inside a
//            wave, the waves' totals are summed through LDS: the drawn cells leave in ASCENDING cell order -- no global atomics, bit-reproducible;
//   rays   : ray n belongs to drawn cell n: a uniform pixel of the cell (utils.py:108-112: the row is "x"), then write_sampled_ray (RGBA: with the blend).
constexpr uint32_t kWeightedThreads = 1024, kWeightedWaves = kWeightedThreads / 64, kMaxErrorGrid = 128, kMaxKeysPerLane = kMaxErrorGrid * kMaxErrorGrid / kWeightedThreads;
constexpr uint32_t kHistCopies = 32;

template <bool RGBA, class Store>
__global__ __launch_bounds__(kWeightedThreads) void k_sample_rays_weighted(SampleBatch b, Store store, const float *__restrict__ error_map, uint32_t G,
                                                                           int64_t *__restrict__ inds_coarse_out, float *__restrict__ keys_out) {
    __shared__ uint32_t hist[256 * kHistCopies];                  // 32 KiB
    __shared__ uint32_t drawn[kMaxErrorGrid * kMaxErrorGrid];     // 64 KiB: the drawn cells in ascending order
    __shared__ uint32_t bins[256];
    __shared__ uint32_t wave_tot[kWeightedWaves];
    __shared__ uint32_t found[2];                                 // the pass's digit, the keys above it

    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t step = b.step(), p = b.pose_of(step), N = b.N, H = b.H, W = b.W;
    const uint32_t cells = G * G, R = ceil_div(cells, kWeightedThreads);
    const uint32_t first = wave * 64u * R + lane;                 // this lane's cells: first + 64 i, i < R

    // ---- keys
    const float *w_row = error_map + (size_t)p * cells;
    const uint32_t key_base = b.base(step, kRaceKeyStream);
    uint32_t key[kMaxKeysPerLane];
#pragma unroll
    for (uint32_t i = 0; i < kMaxKeysPerLane; ++i) {
        const uint32_t c = first + 64u * i;
        key[i] = 0u;
        if (i < R && c < cells) {
            const float w = w_row[c];
            const float u = unit24_open0(draw_word(key_base, c) >> 8);
            const float k = (w > 0.0f && w <= FLT_MAX) ? w / (0.0f - logf(u)) : 0.0f;                // u == 1: w / +0 = +inf
            key[i] = __float_as_uint(k);
            if (keys_out != nullptr) keys_out[c] = k;
        }
    }

    // ---- radix select: `prefix` = the threshold's bits above `shift`, `need` = how many of the keys matching it are still to be taken
    uint32_t prefix = 0u, need = N;
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (uint32_t b = tid; b < 256u * kHistCopies; b += kWeightedThreads) hist[b] = 0u;
        __syncthreads();
#pragma unroll
        for (uint32_t i = 0; i < kMaxKeysPerLane; ++i) {
            const uint32_t c = first + 64u * i;
            if (i < R && c < cells && (shift == 24 || (key[i] >> (shift + 8)) == prefix))
                atomicAdd(&hist[((key[i] >> shift) & 255u) * kHistCopies + (lane & (kHistCopies - 1u))], 1u);
        }
        __syncthreads();
        if (tid < 256u) {
            uint32_t s = 0u;
            for (uint32_t j = 0; j < kHistCopies; ++j) s += hist[tid * kHistCopies + ((j + tid) & (kHistCopies - 1u))];
            bins[tid] = s;
        }
        __syncthreads();
        if (wave == 0u) {       // lane l owns bins 255 - 4 l ... 252 - 4 l: a scan from the top bin down
            uint32_t cnt[4], mine = 0u;
#pragma unroll
            for (uint32_t j = 0; j < 4u; ++j) { cnt[j] = bins[255u - (4u * lane + j)]; mine += cnt[j]; }
            uint32_t run = wave_prefix_sum(mine, (int)lane) - mine;        // keys in the bins above this lane's
#pragma unroll
            for (uint32_t j = 0; j < 4u; ++j) {
                if (run < need && run + cnt[j] >= need) { found[0] = 255u - (4u * lane + j); found[1] = run; }
                run += cnt[j];
            }
        }
        __syncthreads();
        prefix = (prefix << 8) | found[0];
        need -= found[1];
    }
    // prefix = the threshold key T; N - need keys exceed it, and need >= 1 of the keys equal to it are drawn

    // ---- compaction in cell order
    uint32_t n_gt = 0u, n_eq = 0u;
#pragma unroll
    for (uint32_t i = 0; i < kMaxKeysPerLane; ++i) {
        const uint32_t c = first + 64u * i;
        const bool live = i < R && c < cells;
        n_gt += (uint32_t)__popcll(__ballot(live && key[i] > prefix));
        n_eq += (uint32_t)__popcll(__ballot(live && key[i] == prefix));
    }
    if (lane == 0u) wave_tot[wave] = (n_eq << 16) | n_gt;         // (both <= 16384 / 16 = 1024 per wave)
    __syncthreads();
    uint32_t gt_before = 0u, eq_before = 0u;
    for (uint32_t w = 0; w < wave; ++w) { gt_before += wave_tot[w] & 0xffffu; eq_before += wave_tot[w] >> 16; }
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (uint32_t i = 0; i < kMaxKeysPerLane; ++i) {
        const uint32_t c = first + 64u * i;
        const bool live = i < R && c < cells;
        const bool gt_ = live && key[i] > prefix, eq_ = live && key[i] == prefix;
        const unsigned long long m_gt = __ballot(gt_), m_eq = __ballot(eq_);
        const uint32_t g = gt_before + (uint32_t)__popcll(m_gt & below), e = eq_before + (uint32_t)__popcll(m_eq & below);
        if (gt_ || (eq_ && e < need)) {
            const uint32_t pos = g + min(e, need);
            if (pos < N) { drawn[pos] = c; inds_coarse_out[pos] = (int64_t)c; }      // (always true: N cells are drawn; a bound on the store all the same)
        }
        gt_before += (uint32_t)__popcll(m_gt);
        eq_before += (uint32_t)__popcll(m_eq);
    }
    __syncthreads();

    // ---- rays: a uniform pixel inside each drawn cell
    const uint32_t row_base = b.base(step, kRaceRowStream), col_base = b.base(step, kRaceColStream);
    const uint32_t bg_base = RGBA ? b.base(step, kBackgroundStream) : 0u;
    const float sx = (float)H / (float)G, sy = (float)W / (float)G;
    for (uint32_t n = tid; n < N; n += kWeightedThreads) {
        const uint32_t c = drawn[n];
        const float u1 = unit24(draw_word(row_base, n) >> 8), u2 = unit24(draw_word(col_base, n) >> 8);
        const uint32_t row = min(H - 1u, (uint32_t)((float)(c / G) * sx + u1 * sx)), col = min(W - 1u, (uint32_t)((float)(c % G) * sy + u2 * sy));
        write_sampled_ray<RGBA>(b, store, p, row * W + col, n, bg_base);
    }
    if (b.pose_out != nullptr && tid == 0u) b.pose_out[0] = (int32_t)p;
}

// The map's update behind the step's loss (nerf/utils.py:534-556): cell <- 0.1 old + 0.9 error with error = the ray's squared error averaged over the three
// channels.  The cells of one draw are distinct: plain stores.  A non-finite error leaves its cell alone (one NaN pixel would otherwise retire the cell for good).
__global__ void k_error_map_update(float *__restrict__ error_map, uint32_t P, uint32_t cells, const int32_t *__restrict__ pose, const int64_t *__restrict__ inds_coarse,
                                   const float *__restrict__ pred, const float *__restrict__ gt, uint32_t N) {
    const uint32_t n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const uint32_t p = (uint32_t)pose[0];
    const uint64_t c = (uint64_t)inds_coarse[n];
    if (p >= P || c >= cells) return;
    const float d0 = pred[3 * (size_t)n] - gt[3 * (size_t)n], d1 = pred[3 * (size_t)n + 1] - gt[3 * (size_t)n + 1], d2 = pred[3 * (size_t)n + 2] - gt[3 * (size_t)n + 2];
    const float e = (d0 * d0 + d1 * d1 + d2 * d2) / 3.0f;
    if (!(fabsf(e) <= FLT_MAX)) return;
    float *cell = error_map + (size_t)p * cells + c;
    *cell = 0.1f * *cell + 0.9f * e;
}

}  // namespace nsig

// ============================================================================= C ABI
using namespace nsig;

// What every store sampler requires of its batch.  more_pointers: the caller's further required pointers, all present (they share the first refusal).
template <bool RGBA, class Store>
static int check_sample_batch(const char *name, const SampleBatch &b, Store store, bool more_pointers = true) {
    NSIG_REQUIRE(b.poses && b.rays_o && b.rays_d && more_pointers && (!RGBA || (store.px && b.bg_out)), "%s: null pointer", name);
    NSIG_REQUIRE(b.P > 0 && b.H > 0 && b.W > 0 && b.fx != 0.0f && b.fy != 0.0f, "%s: empty pose store, bad image size or focal length", name);
    NSIG_REQUIRE(b.gt == nullptr || store.px != nullptr, "%s: ground truth requested without an image store", name);
    NSIG_REQUIRE((uint64_t)b.H * b.W < (1ull << 32), "%s: image too large", name);
    NSIG_REQUIRE(!RGBA || (Store::kRgbaAlign == 16 ? aligned16(store.px) : aligned4(store.px)), "%s: the RGBA store must be %u-byte aligned", name, Store::kRgbaAlign);
    return NSIG_OK;
}

// rg_sample_rays / rg_sample_rays_rgba / rg_sample_rays_u8: one body, the store's channel count and its pixel fetch as the kernel's template arguments
template <bool RGBA, class Store>
static int sample_rays(const char *name, const SampleBatch &b, Store store, nsig_stream_t stream) {
    if (b.N == 0) return NSIG_OK;
    if (int e = check_sample_batch<RGBA>(name, b, store)) return e;
    k_sample_rays<RGBA><<<ceil_div(b.N, 256u), 256, 0, as_stream(stream)>>>(b, store);
    return check_launch(name);
}

// rg_sample_rays_weighted / _rgba / _u8, likewise
template <bool RGBA, class Store>
static int sample_rays_weighted(const char *name, const SampleBatch &b, Store store, const float *error_map, uint32_t grid, int64_t *inds_coarse_out, float *keys_out,
                                nsig_stream_t stream) {
    if (int e = check_sample_batch<RGBA>(name, b, store, error_map && inds_coarse_out)) return e;
    NSIG_REQUIRE(grid >= 1 && grid <= kMaxErrorGrid, "%s: grid %u out of range (1..%u)", name, grid, kMaxErrorGrid);
    NSIG_REQUIRE(b.N >= 1 && b.N <= grid * grid, "%s: N %u out of range (1..grid * grid = %u: a draw without replacement)", name, b.N, grid * grid);
    k_sample_rays_weighted<RGBA><<<1, kWeightedThreads, 0, as_stream(stream)>>>(b, store, error_map, grid, inds_coarse_out, keys_out);
    return check_launch(name);
}

// the u8 entry points: `channels` picks the template argument the float entry points carry in their names; bg_out goes with an alpha channel, and only with one
#define NSIG_REQUIRE_U8_STORE(name)                                                                                                        \
    NSIG_REQUIRE(channels == 3 || channels == 4, name ": a u8 store holds 3 or 4 channels, not %u", channels);                             \
    NSIG_REQUIRE((channels == 4) == (bg_out != nullptr), name ": bg_out belongs to a 4-channel store, and is required there")

NSIG_EXPORT int rg_sample_rays(const float *poses, uint32_t P, const float *images, float fx, float fy, float cx, float cy, uint32_t H, uint32_t W,
                               uint32_t N, const int32_t *step_counter, uint32_t stride, uint32_t offset, uint64_t seed, float *rays_o, float *rays_d,
                               float *gt, int64_t *inds_out, int32_t *pose_out, nsig_stream_t stream) {
    const SampleBatch b{poses, P, fx, fy, cx, cy, H, W, N, step_counter, stride, offset, (uint32_t)seed, (uint32_t)(seed >> 32), rays_o, rays_d, gt, inds_out, pose_out, nullptr};
    return sample_rays<false>("rg_sample_rays", b, FloatStore{images}, stream);
}

NSIG_EXPORT int rg_sample_rays_rgba(const float *poses, uint32_t P, const float *images, float fx, float fy, float cx, float cy, uint32_t H, uint32_t W,
                                    uint32_t N, const int32_t *step_counter, uint32_t stride, uint32_t offset, uint64_t seed, float *rays_o, float *rays_d,
                                    float *gt, float *bg_out, int64_t *inds_out, int32_t *pose_out, nsig_stream_t stream) {
    const SampleBatch b{poses, P, fx, fy, cx, cy, H, W, N, step_counter, stride, offset, (uint32_t)seed, (uint32_t)(seed >> 32), rays_o, rays_d, gt, inds_out, pose_out, bg_out};
    return sample_rays<true>("rg_sample_rays_rgba", b, FloatStore{images}, stream);
}

NSIG_EXPORT int rg_sample_rays_u8(const float *poses, uint32_t P, const uint8_t *images, uint32_t channels, const float *decode, float fx, float fy, float cx, float cy,
                                  uint32_t H, uint32_t W, uint32_t N, const int32_t *step_counter, uint32_t stride, uint32_t offset, uint64_t seed, float *rays_o,
                                  float *rays_d, float *gt, float *bg_out, int64_t *inds_out, int32_t *pose_out, nsig_stream_t stream) {
    NSIG_REQUIRE_U8_STORE("rg_sample_rays_u8");
    const U8Store store{images, decode};
    const SampleBatch b{poses, P, fx, fy, cx, cy, H, W, N, step_counter, stride, offset, (uint32_t)seed, (uint32_t)(seed >> 32), rays_o, rays_d, gt, inds_out, pose_out, bg_out};
    return channels == 4 ? sample_rays<true>("rg_sample_rays_u8", b, store, stream) : sample_rays<false>("rg_sample_rays_u8", b, store, stream);
}

NSIG_EXPORT int rg_sample_rays_orbit(float fx, float fy, float cx, float cy, uint32_t H, uint32_t W, uint32_t N, const int32_t *step_counter, uint32_t stride,
                                     uint32_t offset, uint64_t seed, float radius, float theta0, float theta1, float phi0, float phi1, float *rays_o, float *rays_d,
                                     int64_t *inds_out, float *pose_out, nsig_stream_t stream) {
    NSIG_REQUIRE(rays_o && rays_d && pose_out, "rg_sample_rays_orbit: null pointer");
    NSIG_REQUIRE(N >= 1, "rg_sample_rays_orbit: N must be at least 1 (lane 0 writes the pose)");
    NSIG_REQUIRE(H > 0 && W > 0 && fx != 0.0f && fy != 0.0f, "rg_sample_rays_orbit: bad image size or focal length");
    NSIG_REQUIRE((uint64_t)H * W < (1ull << 32), "rg_sample_rays_orbit: image too large");
    NSIG_REQUIRE(radius > 0.0f && theta0 <= theta1 && phi0 <= phi1, "rg_sample_rays_orbit: radius must be positive and the angle ranges ordered");
    NSIG_REQUIRE(theta0 > 0.0f && theta1 < 3.14159265f, "rg_sample_rays_orbit: polar angles must lie strictly inside (0, pi): the look-at frame is undefined at the poles");
    const SampleBatch b{nullptr, 0u, fx, fy, cx, cy, H, W, N, step_counter, stride, offset, (uint32_t)seed, (uint32_t)(seed >> 32), rays_o, rays_d, nullptr, inds_out, nullptr, nullptr};
    k_sample_rays_orbit<<<ceil_div(N, 256u), 256, 0, as_stream(stream)>>>(b, OrbitRange{radius, theta0, theta1, phi0, phi1}, pose_out);
    return check_launch("rg_sample_rays_orbit");
}

NSIG_EXPORT int rg_sample_rays_weighted(const float *poses, uint32_t P, const float *images, float fx, float fy, float cx, float cy, uint32_t H, uint32_t W,
                                        uint32_t N, const int32_t *step_counter, uint32_t stride, uint32_t offset, uint64_t seed, const float *error_map, uint32_t grid,
                                        float *rays_o, float *rays_d, float *gt, int64_t *inds_out, int32_t *pose_out, int64_t *inds_coarse_out, float *keys_out,
                                        nsig_stream_t stream) {
    const SampleBatch b{poses, P, fx, fy, cx, cy, H, W, N, step_counter, stride, offset, (uint32_t)seed, (uint32_t)(seed >> 32), rays_o, rays_d, gt, inds_out, pose_out, nullptr};
    return sample_rays_weighted<false>("rg_sample_rays_weighted", b, FloatStore{images}, error_map, grid, inds_coarse_out, keys_out, stream);
}

NSIG_EXPORT int rg_sample_rays_weighted_rgba(const float *poses, uint32_t P, const float *images, float fx, float fy, float cx, float cy, uint32_t H, uint32_t W,
                                             uint32_t N, const int32_t *step_counter, uint32_t stride, uint32_t offset, uint64_t seed, const float *error_map,
                                             uint32_t grid, float *rays_o, float *rays_d, float *gt, float *bg_out, int64_t *inds_out, int32_t *pose_out,
                                             int64_t *inds_coarse_out, float *keys_out, nsig_stream_t stream) {
    const SampleBatch b{poses, P, fx, fy, cx, cy, H, W, N, step_counter, stride, offset, (uint32_t)seed, (uint32_t)(seed >> 32), rays_o, rays_d, gt, inds_out, pose_out, bg_out};
    return sample_rays_weighted<true>("rg_sample_rays_weighted_rgba", b, FloatStore{images}, error_map, grid, inds_coarse_out, keys_out, stream);
}

NSIG_EXPORT int rg_sample_rays_weighted_u8(const float *poses, uint32_t P, const uint8_t *images, uint32_t channels, const float *decode, float fx, float fy, float cx,
                                           float cy, uint32_t H, uint32_t W, uint32_t N, const int32_t *step_counter, uint32_t stride, uint32_t offset, uint64_t seed,
                                           const float *error_map, uint32_t grid, float *rays_o, float *rays_d, float *gt, float *bg_out, int64_t *inds_out,
                                           int32_t *pose_out, int64_t *inds_coarse_out, float *keys_out, nsig_stream_t stream) {
    NSIG_REQUIRE_U8_STORE("rg_sample_rays_weighted_u8");
    const U8Store store{images, decode};
    const SampleBatch b{poses, P, fx, fy, cx, cy, H, W, N, step_counter, stride, offset, (uint32_t)seed, (uint32_t)(seed >> 32), rays_o, rays_d, gt, inds_out, pose_out, bg_out};
    return channels == 4 ? sample_rays_weighted<true>("rg_sample_rays_weighted_u8", b, store, error_map, grid, inds_coarse_out, keys_out, stream)
                         : sample_rays_weighted<false>("rg_sample_rays_weighted_u8", b, store, error_map, grid, inds_coarse_out, keys_out, stream);
}
#undef NSIG_REQUIRE_U8_STORE

NSIG_EXPORT int rg_blend_random_background(const float *rgba, uint32_t N, const int32_t *step_counter, uint64_t seed, float *bg_out, float *gt_out,
                                           nsig_stream_t stream) {
    if (N == 0) return NSIG_OK;
    NSIG_REQUIRE(rgba && bg_out && gt_out, "rg_blend_random_background: null pointer");
    NSIG_REQUIRE(aligned16(rgba), "rg_blend_random_background: rgba must be 16-byte aligned");
    k_blend_random_background<<<ceil_div(N, 256u), 256, 0, as_stream(stream)>>>(reinterpret_cast<const float4 *>(rgba), N, step_counter, (uint32_t)seed,
                                                                                (uint32_t)(seed >> 32), bg_out, gt_out);
    return check_launch("rg_blend_random_background");
}

NSIG_EXPORT int rg_error_map_update(float *error_map, uint32_t P, uint32_t grid, const int32_t *pose_dev, const int64_t *inds_coarse, const float *pred,
                                    const float *gt, uint32_t N, nsig_stream_t stream) {
    if (N == 0) return NSIG_OK;
    NSIG_REQUIRE(error_map && pose_dev && inds_coarse && pred && gt, "rg_error_map_update: null pointer");
    NSIG_REQUIRE(P > 0 && grid >= 1 && grid <= kMaxErrorGrid, "rg_error_map_update: empty map or grid %u out of range (1..%u)", grid, kMaxErrorGrid);
    k_error_map_update<<<ceil_div(N, 256u), 256, 0, as_stream(stream)>>>(error_map, P, grid * grid, pose_dev, inds_coarse, pred, gt, N);
    return check_launch("rg_error_map_update");
}

NSIG_EXPORT int rg_get_rays(const float *poses, float fx, float fy, float cx, float cy, uint32_t H, uint32_t W, const int64_t *inds,
                            uint32_t B, uint32_t N, float *rays_o, float *rays_d, nsig_stream_t stream) {
    NSIG_REQUIRE(poses && rays_o && rays_d, "rg_get_rays: null pointer");
    NSIG_REQUIRE(H > 0 && W > 0 && fx != 0.0f && fy != 0.0f, "rg_get_rays: bad image size or focal length");
    NSIG_REQUIRE(inds != nullptr || N == H * W, "rg_get_rays: without indices N must equal H*W");
    NSIG_REQUIRE((uint64_t)B * N < (1ull << 32), "rg_get_rays: too many rays");
    if (B * N == 0) return NSIG_OK;
    k_get_rays<<<ceil_div(B * N, 256), 256, 0, as_stream(stream)>>>(poses, fx, fy, cx, cy, H, W, inds, B, N, rays_o, rays_d);
    return check_launch("rg_get_rays");
}
