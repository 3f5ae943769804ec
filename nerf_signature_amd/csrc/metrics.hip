// Image metrics of rendered views on the device: value range + squared error in one pass, SSIM in one pass (replaces, for this project's own
// evaluation, the reference's PSNRMeter / SSIMMeter of nerf/utils_wtmk_disen.py:211-282; SSIM restates torchmetrics'
// structural_similarity_index_measure with every default -- DESIGN.md section 15).
//
// Images are contiguous fp32 [B, H, W, C], channel last, as the renderer writes them.
//   range + SSE: grid (nb, B); every workgroup strides over its image and stores min/max of both tensors and sum (double)(float(p - t))^2;
//                the finish launch takes the extrema over all B nb partials and adds each image's nb partials in a fixed order.
//   SSIM:        a workgroup owns a 32 x 16 tile of the (H-10) x (W-10) map.  It stages the 42 x 26 window of both images (all channels) in LDS,
//                as differences from a per-tile, per-channel shift (variance and covariance do not see a shift; E[pp] - E[p]^2 cancels far less
//                about a nearby value than about 0), and then per channel filters 11 taps along x into LDS (6 moments) and 11 along y out of
//                it, evaluates the formula and reduces its tile in double.  Every window of the cropped map lies inside the image: no padding.
//                The covariance is taken through the variance of the difference d = p - t: 2 cov = var p + var t - var d, so
//                2 cov + c2 = (var p + var t + c2) - var d and ssim's second factor is 1 - var d / (var p + var t + c2).  d is small where the
//                images are close, var d = E[dd] - E[d]^2 then does not cancel, and the rounding of var p + var t (about 1e-8, against
//                c2 = 9e-4) only enters scaled by var d / (var p + var t + c2).  Computed directly, E[pt] - E[p]E[t] carries that rounding in
//                full and independently of the two variances': 1e-5 per window, and one-sided where a clamped variance meets an unclamped
//                covariance.  All three variances are clamped at 0 (the definition clamps var p and var t; var d >= 0 likewise).
//                The finish launch adds each image's tile partials in a fixed order and divides by C (H-10) (W-10).
// No atomics anywhere: the same inputs give the same bits.  pred and truth enter every expression symmetrically: swapping them changes no bit.
#include <math.h>

#include "wave.h"

namespace nsig {

constexpr uint32_t kImThreads = 256;      // 4 waves
constexpr uint32_t kImRangeMaxBlocks = 256;   // per image: one partial per thread of the finish launch
constexpr uint32_t kImRangePerBlock = kImThreads * 16;
constexpr int kWin = 11, kHalo = kWin - 1;
constexpr int kMoments = 6;      // of p, t, p p, t t, d, d d with d = p - t
constexpr int kTileX = 32, kTileY = 16, kInX = kTileX + kHalo, kInY = kTileY + kHalo;
constexpr uint32_t kImMaxSide = 1u << 15, kImMaxBatch = 65535;

struct SsimWindow {
    float g[kWin];
};

static inline size_t im_align(size_t b) { return (b + 255) & ~size_t(255); }

static inline uint32_t range_blocks(uint64_t n) {
    const uint64_t nb = (n + kImRangePerBlock - 1) / kImRangePerBlock;
    return (uint32_t)(nb < 1 ? 1 : nb > kImRangeMaxBlocks ? kImRangeMaxBlocks : nb);
}

// range scratch: ext[4][B nb] float (pred min, pred max, truth min, truth max), sse[B nb] double
struct RangeScratch {
    float *ext;
    double *sse;
    uint32_t nb;
};
static inline size_t range_bytes(uint32_t B, uint64_t n) {
    const size_t e = size_t(B) * range_blocks(n);
    return im_align(e * 16) + im_align(e * 8);
}
static inline RangeScratch range_split(void *scratch, uint32_t B, uint64_t n) {
    RangeScratch s;
    s.nb = range_blocks(n);
    s.ext = static_cast<float *>(scratch);
    s.sse = reinterpret_cast<double *>(static_cast<char *>(scratch) + im_align(size_t(B) * s.nb * 16));
    return s;
}

// Sum over the workgroup in a fixed order (wave butterfly, then the waves in index order); the result is valid in thread 0.
__device__ inline double block_sum(double v, double *red) {
    const uint32_t tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    v = wave_sum(v);
    if (lane == 0) red[wid] = v;
    __syncthreads();
    double s = 0.0;
    if (tid == 0) {
#pragma unroll
        for (uint32_t w = 0; w < kImThreads / kWave; ++w) s += red[w];
    }
    __syncthreads();
    return s;
}

__device__ inline float block_min(float v, float *red) {
    const uint32_t tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    v = wave_min(v);
    if (lane == 0) red[wid] = v;
    __syncthreads();
    float s = v;
    if (tid == 0) {
#pragma unroll
        for (uint32_t w = 0; w < kImThreads / kWave; ++w) s = fminf(s, red[w]);
    }
    __syncthreads();
    return s;
}

struct RangeAcc {
    float pmin, pmax, tmin, tmax;
    double sse;
    __device__ inline void add(float p, float t) {
        pmin = fminf(pmin, p);
        pmax = fmaxf(pmax, p);
        tmin = fminf(tmin, t);
        tmax = fmaxf(tmax, t);
        const double d = (double)(p - t);
        sse += d * d;
    }
};

// Pass 1: image blockIdx.y, elements [0, n).  vec: n is a multiple of 4 and both bases are 16-byte aligned (16-byte loads).
__global__ void __launch_bounds__(kImThreads) k_im_range(const float *__restrict__ pred, const float *__restrict__ truth, uint64_t n, int vec,
                                                         float *__restrict__ ext, double *__restrict__ sse) {
    __shared__ double red_d[kImThreads / kWave];
    __shared__ float red_f[kImThreads / kWave];
    const uint32_t nb = gridDim.x, E = gridDim.y * nb, slot = blockIdx.y * nb + blockIdx.x;
    const float *p = pred + (size_t)blockIdx.y * n, *t = truth + (size_t)blockIdx.y * n;
    RangeAcc a{INFINITY, -INFINITY, INFINITY, -INFINITY, 0.0};
    const uint64_t first = (uint64_t)blockIdx.x * kImThreads + threadIdx.x, step = (uint64_t)nb * kImThreads;
    if (vec) {
        const float4 *p4 = reinterpret_cast<const float4 *>(p), *t4 = reinterpret_cast<const float4 *>(t);
        for (uint64_t i = first; i < n / 4; i += step) {
            const float4 x = p4[i], y = t4[i];
            a.add(x.x, y.x);
            a.add(x.y, y.y);
            a.add(x.z, y.z);
            a.add(x.w, y.w);
        }
    } else {
        for (uint64_t i = first; i < n; i += step) a.add(p[i], t[i]);
    }
    const float pmin = block_min(a.pmin, red_f), pmax = -block_min(-a.pmax, red_f);
    const float tmin = block_min(a.tmin, red_f), tmax = -block_min(-a.tmax, red_f);
    const double s = block_sum(a.sse, red_d);
    if (threadIdx.x == 0) {
        ext[slot] = pmin;
        ext[E + slot] = pmax;
        ext[2 * E + slot] = tmin;
        ext[3 * E + slot] = tmax;
        sse[slot] = s;
    }
}

// Pass 1 finish: workgroup b adds image b's nb <= 256 partials (thread i holds partial i); workgroup 0 also takes the extrema of all B nb.
__global__ void __launch_bounds__(kImThreads) k_im_range_finish(const float *__restrict__ ext, const double *__restrict__ sse, uint32_t nb, uint32_t B,
                                                                float *__restrict__ extrema, double *__restrict__ sse_out) {
    __shared__ double red_d[kImThreads / kWave];
    __shared__ float red_f[kImThreads / kWave];
    const uint32_t tid = threadIdx.x, b = blockIdx.x, E = B * nb;
    const double s = block_sum(tid < nb ? sse[b * nb + tid] : 0.0, red_d);
    if (tid == 0) sse_out[b] = s;
    if (b != 0) return;
    float v[4] = {INFINITY, INFINITY, INFINITY, INFINITY};      // (maxima negated)
    for (uint32_t i = tid; i < E; i += kImThreads) {
        v[0] = fminf(v[0], ext[i]);
        v[1] = fminf(v[1], -ext[E + i]);
        v[2] = fminf(v[2], ext[2 * E + i]);
        v[3] = fminf(v[3], -ext[3 * E + i]);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float m = block_min(v[k], red_f);
        if (tid == 0) extrema[k] = (k & 1) ? -m : m;
    }
}

// Pass 2.  grid (tiles x, tiles y, B); partial[b][tile] = the tile's sum of ssim over its pixels and channels.
template <int C>
__global__ void __launch_bounds__(kImThreads) k_im_ssim(const float *__restrict__ pred, const float *__restrict__ truth, uint32_t H, uint32_t W,
                                                        const float *__restrict__ extrema, float data_range, SsimWindow win,
                                                        double *__restrict__ partial, float *__restrict__ map) {
    __shared__ float in_p[kInY][kInX * C], in_t[kInY][kInX * C];
    __shared__ float hb[kMoments][kInY][kTileX];
    __shared__ float shift[C];
    __shared__ double red_d[kImThreads / kWave];
    const uint32_t tid = threadIdx.x;
    const uint32_t x0 = blockIdx.x * kTileX, y0 = blockIdx.y * kTileY, b = blockIdx.z;
    const uint32_t OH = H - kHalo, OW = W - kHalo;
    const float *p = pred + (size_t)b * H * W * C, *t = truth + (size_t)b * H * W * C;

    float dr = data_range;
    if (extrema) dr = fmaxf(extrema[1] - extrema[0], extrema[3] - extrema[2]);
    const double r1 = 0.01 * (double)dr, r2 = 0.03 * (double)dr;
    const float c1 = (float)(r1 * r1), c2 = (float)(r2 * r2);

    if (tid < C) shift[tid] = 0.5f * (p[((size_t)y0 * W + x0) * C + tid] + t[((size_t)y0 * W + x0) * C + tid]);      // (y0, x0) is inside the image
    __syncthreads();
    // stage: rows of kInX * C contiguous floats; outside the image -> 0 (such entries reach only outputs outside the map)
    for (uint32_t i = tid; i < kInY * kInX * C; i += kImThreads) {
        const uint32_t r = i / (kInX * C), q = i % (kInX * C), y = y0 + r, x = x0 + q / C;
        float a = 0.0f, c = 0.0f;
        if (y < H && x < W) {
            const size_t g = ((size_t)y * W + x0) * C + q;
            const float s = shift[q % C];
            a = p[g] - s;
            c = t[g] - s;
        }
        in_p[r][q] = a;
        in_t[r][q] = c;
    }
    __syncthreads();

    double acc = 0.0;
    for (int ch = 0; ch < C; ++ch) {
        // along x: the moments of every staged row at the tile's 32 columns
        for (uint32_t i = tid; i < kInY * kTileX; i += kImThreads) {
            const uint32_t r = i / kTileX, x = i % kTileX;
            float sp = 0.0f, st = 0.0f, spp = 0.0f, stt = 0.0f, sd = 0.0f, sdd = 0.0f;
#pragma unroll
            for (int k = 0; k < kWin; ++k) {
                const float w = win.g[k], a = in_p[r][(x + k) * C + ch], c = in_t[r][(x + k) * C + ch], d = a - c;
                sp = fmaf(w, a, sp);
                st = fmaf(w, c, st);
                spp = fmaf(w, a * a, spp);
                stt = fmaf(w, c * c, stt);
                sd = fmaf(w, d, sd);
                sdd = fmaf(w, d * d, sdd);
            }
            hb[0][r][x] = sp;
            hb[1][r][x] = st;
            hb[2][r][x] = spp;
            hb[3][r][x] = stt;
            hb[4][r][x] = sd;
            hb[5][r][x] = sdd;
        }
        __syncthreads();
        // along y, the formula, the tile's sum
        const float s = shift[ch];
#pragma unroll
        for (uint32_t j = 0; j < kTileX * kTileY / kImThreads; ++j) {
            const uint32_t x = tid % kTileX, y = tid / kTileX + j * (kImThreads / kTileX);
            float m[kMoments] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int k = 0; k < kWin; ++k) {
                const float w = win.g[k];
#pragma unroll
                for (int q = 0; q < kMoments; ++q) m[q] = fmaf(w, hb[q][y + k][x], m[q]);
            }
            const float vp = fmaxf(m[2] - m[0] * m[0], 0.0f), vt = fmaxf(m[3] - m[1] * m[1], 0.0f), vd = fmaxf(m[5] - m[4] * m[4], 0.0f);
            const float mp = m[0] + s, mt = m[1] + s, vs = (vp + vt) + c2;
            const float num = (2.0f * (mp * mt) + c1) * (vs - vd);      // 2 cov + c2
            const float den = ((mp * mp + mt * mt) + c1) * vs;
            const float v = num / den;
            if (y0 + y < OH && x0 + x < OW) {
                acc += (double)v;
                if (map) map[(((size_t)b * OH + (y0 + y)) * OW + (x0 + x)) * C + ch] = v;
            }
        }
        __syncthreads();
    }
    const double sum = block_sum(acc, red_d);
    if (tid == 0) partial[(size_t)b * gridDim.x * gridDim.y + blockIdx.y * gridDim.x + blockIdx.x] = sum;
}

// Pass 2 finish: workgroup b adds image b's nt tile partials -- thread i those of index i, i + 256, ... in rising order, then the fixed
// workgroup order -- and divides by the number of map values.
__global__ void __launch_bounds__(kImThreads) k_im_ssim_finish(const double *__restrict__ partial, uint32_t nt, double count, double *__restrict__ ssim) {
    __shared__ double red_d[kImThreads / kWave];
    const uint32_t b = blockIdx.x;
    double s = 0.0;
    for (uint32_t i = threadIdx.x; i < nt; i += kImThreads) s += partial[(size_t)b * nt + i];
    s = block_sum(s, red_d);
    if (threadIdx.x == 0) ssim[b] = s / count;
}

static inline bool ssim_dims_ok(uint32_t B, uint32_t H, uint32_t W, uint32_t C) {
    return B >= 1 && B <= kImMaxBatch && C >= 1 && C <= 4 && H >= (uint32_t)kWin && W >= (uint32_t)kWin && H <= kImMaxSide && W <= kImMaxSide;
}
static inline uint32_t ssim_tiles_x(uint32_t W) { return ceil_div(W - kHalo, kTileX); }
static inline uint32_t ssim_tiles_y(uint32_t H) { return ceil_div(H - kHalo, kTileY); }

static SsimWindow make_window() {      // g[i] = exp(-((i - 5) / 1.5)^2 / 2), normalised to sum 1 in double, rounded once
    double g[kWin], sum = 0.0;
    for (int i = 0; i < kWin; ++i) {
        const double d = (i - kWin / 2) / 1.5;
        g[i] = exp(-0.5 * d * d);
        sum += g[i];
    }
    SsimWindow w;
    for (int i = 0; i < kWin; ++i) w.g[i] = (float)(g[i] / sum);
    return w;
}

}  // namespace nsig

using namespace nsig;

NSIG_EXPORT size_t im_range_scratch_bytes(uint32_t B, uint64_t n) {
    if (B < 1 || B > kImMaxBatch || n < 1) return 0;
    return range_bytes(B, n);
}

NSIG_EXPORT int im_range_sse(const float *pred, const float *truth, uint32_t B, uint64_t n, void *scratch, float *extrema, double *sse, nsig_stream_t stream) {
    NSIG_REQUIRE(pred && truth && scratch && extrema && sse, "im_range_sse: null pointer");
    NSIG_REQUIRE(B >= 1 && B <= kImMaxBatch, "im_range_sse: batch of %u images is out of range (1 .. %u)", B, kImMaxBatch);
    NSIG_REQUIRE(n >= 1 && n <= (1ull << 40), "im_range_sse: %llu values per image is out of range", (unsigned long long)n);
    NSIG_REQUIRE(aligned16(scratch), "im_range_sse: scratch must be 16-byte aligned");
    const RangeScratch s = range_split(scratch, B, n);
    const int vec = n % 4 == 0 && aligned16(pred) && aligned16(truth);
    k_im_range<<<dim3(s.nb, B), kImThreads, 0, as_stream(stream)>>>(pred, truth, n, vec, s.ext, s.sse);
    k_im_range_finish<<<B, kImThreads, 0, as_stream(stream)>>>(s.ext, s.sse, s.nb, B, extrema, sse);
    return check_launch("im_range_sse");
}

NSIG_EXPORT size_t im_ssim_scratch_bytes(uint32_t B, uint32_t H, uint32_t W, uint32_t C) {
    if (!ssim_dims_ok(B, H, W, C)) return 0;
    return im_align(size_t(B) * ssim_tiles_x(W) * ssim_tiles_y(H) * 8);
}

NSIG_EXPORT int im_ssim(const float *pred, const float *truth, uint32_t B, uint32_t H, uint32_t W, uint32_t C, const float *extrema, float data_range,
                        void *scratch, double *ssim, float *map, nsig_stream_t stream) {
    NSIG_REQUIRE(pred && truth && scratch && ssim, "im_ssim: null pointer");
    NSIG_REQUIRE(B >= 1 && B <= kImMaxBatch, "im_ssim: batch of %u images is out of range (1 .. %u)", B, kImMaxBatch);
    NSIG_REQUIRE(C >= 1 && C <= 4, "im_ssim: %u channels is out of range (1 .. 4)", C);
    NSIG_REQUIRE(H >= (uint32_t)kWin && W >= (uint32_t)kWin && H <= kImMaxSide && W <= kImMaxSide,
                 "im_ssim: image of %u x %u pixels is out of range (each side %d .. %u: one 11 x 11 window at least)", H, W, kWin, kImMaxSide);
    NSIG_REQUIRE(extrema || data_range >= 0.0f, "im_ssim: without device extrema the data range must be a number >= 0");
    NSIG_REQUIRE(aligned16(scratch), "im_ssim: scratch must be 16-byte aligned");
    const uint32_t gx = ssim_tiles_x(W), gy = ssim_tiles_y(H);
    const dim3 grid(gx, gy, B);
    const SsimWindow win = make_window();
    double *partial = static_cast<double *>(scratch);
    hipStream_t st = as_stream(stream);
    switch (C) {
        case 1: k_im_ssim<1><<<grid, kImThreads, 0, st>>>(pred, truth, H, W, extrema, data_range, win, partial, map); break;
        case 2: k_im_ssim<2><<<grid, kImThreads, 0, st>>>(pred, truth, H, W, extrema, data_range, win, partial, map); break;
        case 3: k_im_ssim<3><<<grid, kImThreads, 0, st>>>(pred, truth, H, W, extrema, data_range, win, partial, map); break;
        default: k_im_ssim<4><<<grid, kImThreads, 0, st>>>(pred, truth, H, W, extrema, data_range, win, partial, map); break;
    }
    k_im_ssim_finish<<<B, kImThreads, 0, st>>>(partial, gx * gy, (double)C * (double)(H - kHalo) * (double)(W - kHalo), ssim);
    return check_launch("im_ssim");
}
