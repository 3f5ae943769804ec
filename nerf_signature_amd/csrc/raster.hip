// Triangle rasteriser for exported meshes (include/nerfsig.h, "mesh rasteriser"; restated in tests/raster_ref.py).
//
// rs_project: world vertices -> screen records (x, y on the 1/256 pixel grid, 1 / z, flag), z-buffer and status words reset, one launch.
// rs_raster:  per triangle integer coverage, float64 depth and a 64-bit (depth bits, triangle index) atomicMin per covered pixel centre.  Two launches:
//             k_rs_small -- one lane per triangle walks its clamped box when the box holds at most NSIG_RASTER_SMALL_BOX centres, otherwise the lane appends
//             the triangle to a list (one ballot and one atomic add per wave); k_rs_large -- a fixed grid of waves strides that list, whose length it reads
//             from device memory, one wave per listed triangle, the lanes striding the box.  Both call rs_cover (the one coverage-and-depth body).
// rs_shade:   one lane per pixel; the winner's weights are recomputed by the same rs_setup / rs_cover and the colours interpolated in float64.
//
// The minimum does not depend on arrival order, so neither does any output bit; the order of the large list does, and nothing depends on it.
// No thread waits for another, no loop's trip count depends on another thread, nothing is allocated and no device value is read on the host.
// The library is built with -ffp-contract=off (build.py's BASE_FLAGS): every float and double operation below is rounded on its own.
#include "wave.h"

namespace nsig {

constexpr uint32_t kRsThreads = 256;                 // 4 waves
constexpr uint32_t kRsLargeBlocks = 4 * kCUs;        // k_rs_large's fixed grid: 4096 waves
constexpr uint32_t kRsMaxSide = 4096;
constexpr uint32_t kRsStatusBytes = 256;             // word 0: first bad triangle or kRsNoError, 1: near-plane culls, 2: guard-band culls, 3: length of the large list
constexpr uint32_t kRsNoError = 0xffffffffu;
constexpr unsigned long long kRsEmpty = ~0ull;
constexpr float kRsGuard = NSIG_RASTER_GUARD_PIXELS;
constexpr int32_t kRsHalf = 128, kRsOne = 256;       // 8 sub-pixel bits

struct alignas(16) RsRecord {      // one 128-bit load
    int32_t x, y;      // rintf(u * 256), rintf(v * 256); 0 when flagged
    float iz;          // 1 / Zc; 0 when flagged
    uint32_t flag;     // 0 drawn, 1 behind the near plane (or NaN), 2 outside the guard band
};
static_assert(sizeof(RsRecord) == 16, "screen record");

static inline size_t rs_align(size_t b) { return (b + 255) & ~size_t(255); }

struct RsScratch {
    uint32_t *status;
    RsRecord *rec;
    unsigned long long *zbuf;
    uint32_t *list;
};
static inline size_t rs_bytes(uint32_t V, uint32_t T, uint32_t H, uint32_t W) {
    return kRsStatusBytes + rs_align(size_t(V) * 16) + rs_align(size_t(H) * W * 8) + rs_align(size_t(T) * 4);
}
static inline RsScratch rs_split(void *scratch, uint32_t V, uint32_t H, uint32_t W) {
    char *p = static_cast<char *>(scratch);
    RsScratch s;
    s.status = reinterpret_cast<uint32_t *>(p);
    s.rec = reinterpret_cast<RsRecord *>(p + kRsStatusBytes);
    s.zbuf = reinterpret_cast<unsigned long long *>(p + kRsStatusBytes + rs_align(size_t(V) * 16));
    s.list = reinterpret_cast<uint32_t *>(p + kRsStatusBytes + rs_align(size_t(V) * 16) + rs_align(size_t(H) * W * 8));
    return s;
}

// ---- projection -------------------------------------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(kRsThreads) k_rs_project(const float *__restrict__ verts, uint32_t V, const float *__restrict__ pose, float fx, float fy, float cx,
                                                           float cy, float near, RsRecord *__restrict__ rec, unsigned long long *__restrict__ zbuf, uint32_t npix,
                                                           uint32_t *__restrict__ status) {
    const uint32_t g = blockIdx.x * kRsThreads + threadIdx.x;
    if (g < 4) status[g] = g == 0 ? kRsNoError : 0u;
    if (g < npix) zbuf[g] = kRsEmpty;
    if (g >= V) return;
    const float d0 = verts[3 * (size_t)g] - pose[3], d1 = verts[3 * (size_t)g + 1] - pose[7], d2 = verts[3 * (size_t)g + 2] - pose[11];
    const float Xc = (pose[0] * d0 + pose[4] * d1) + pose[8] * d2;       // R^T d: column 0 of R
    const float Yc = (pose[1] * d0 + pose[5] * d1) + pose[9] * d2;
    const float Zc = (pose[2] * d0 + pose[6] * d1) + pose[10] * d2;
    RsRecord r = {0, 0, 0.0f, 0u};
    if (!(Zc >= near)) {
        r.flag = 1u;
    } else {
        const float u = fx * (Xc / Zc) + cx, v = fy * (Yc / Zc) + cy;
        if (!(fabsf(u) <= kRsGuard) || !(fabsf(v) <= kRsGuard)) {          // (NaN and infinity land here)
            r.flag = 2u;
        } else {
            r.x = (int32_t)rintf(u * 256.0f);                              // round half to even; |u * 256| <= 2^22
            r.y = (int32_t)rintf(v * 256.0f);
            r.iz = 1.0f / Zc;
        }
    }
    rec[g] = r;
}

// ---- the shared triangle body ---------------------------------------------------------------------------------------------------------------------------

// A triangle ready to be drawn: vertices a, b, c with b and c swapped where the signed area was negative (A2 > 0 afterwards), its clamped box of pixel indices.
struct RsTri {
    int32_t id[3];
    int32_t x[3], y[3];
    double iz[3];
    long long A2;
    int32_t i0, i1, j0, j1;      // columns i0 .. i1, rows j0 .. j1 (empty when i0 > i1 or j0 > j1)
};

enum RsFate : uint32_t { kRsDraw = 0, kRsBadId = 1, kRsNear = 2, kRsGuardBand = 3, kRsNoArea = 4 };

// Loads triangle t and classifies it in the header's order: bad id, culled vertex (near before guard), zero area.  Nothing is dereferenced through a bad id.
__device__ inline RsFate rs_setup(const int32_t *__restrict__ tris, uint32_t t, uint32_t V, const RsRecord *__restrict__ rec, uint32_t H, uint32_t W, RsTri &tri) {
    const int32_t a = tris[3 * (size_t)t], b = tris[3 * (size_t)t + 1], c = tris[3 * (size_t)t + 2];
    if ((uint32_t)a >= V || (uint32_t)b >= V || (uint32_t)c >= V) return kRsBadId;      // (negative ids wrap above 2^31 > V)
    const RsRecord ra = rec[a], rb = rec[b], rc = rec[c];
    if (ra.flag == 1u || rb.flag == 1u || rc.flag == 1u) return kRsNear;
    if (ra.flag | rb.flag | rc.flag) return kRsGuardBand;
    const long long A2 = (long long)(rb.x - ra.x) * (rc.y - ra.y) - (long long)(rb.y - ra.y) * (rc.x - ra.x);
    if (A2 == 0) return kRsNoArea;
    const bool swap = A2 < 0;
    const RsRecord &r1 = swap ? rc : rb, &r2 = swap ? rb : rc;
    tri.id[0] = a, tri.id[1] = swap ? c : b, tri.id[2] = swap ? b : c;
    tri.x[0] = ra.x, tri.x[1] = r1.x, tri.x[2] = r2.x;
    tri.y[0] = ra.y, tri.y[1] = r1.y, tri.y[2] = r2.y;
    tri.iz[0] = (double)ra.iz, tri.iz[1] = (double)r1.iz, tri.iz[2] = (double)r2.iz;
    tri.A2 = swap ? -A2 : A2;
    const int32_t xmin = min(ra.x, min(rb.x, rc.x)), xmax = max(ra.x, max(rb.x, rc.x));
    const int32_t ymin = min(ra.y, min(rb.y, rc.y)), ymax = max(ra.y, max(rb.y, rc.y));
    // pixel i has its centre at 256 i + 128: the first centre >= xmin and the last <= xmax (arithmetic shifts: floor division of negatives too)
    tri.i0 = max((xmin + (kRsOne - kRsHalf - 1)) >> 8, 0), tri.i1 = min((xmax - kRsHalf) >> 8, (int32_t)W - 1);
    tri.j0 = max((ymin + (kRsOne - kRsHalf - 1)) >> 8, 0), tri.j1 = min((ymax - kRsHalf) >> 8, (int32_t)H - 1);
    return kRsDraw;
}

// The edge function of the directed edge p -> q at (x, y), and whether a centre exactly on it belongs to this triangle.  With A2 > 0 and y pointing down the
// vertices run clockwise on the screen: a top edge is horizontal and runs right (dy == 0, dx > 0), a left edge runs up (dy < 0).  The neighbour across a
// shared edge walks it the other way, so exactly one of the two owns it.
__device__ inline bool rs_edge(int32_t px, int32_t py, int32_t qx, int32_t qy, int32_t x, int32_t y, long long &E) {
    const int32_t dx = qx - px, dy = qy - py;
    E = (long long)dx * (y - py) - (long long)dy * (x - px);
    return E > 0 || (E == 0 && (dy < 0 || (dy == 0 && dx > 0)));
}

// Coverage of pixel (i, j) and the barycentric weights b_k = E_k / A2 (E_k: the edge opposite vertex k) and q = sum b_k iz_k, in float64.
__device__ inline bool rs_cover(const RsTri &tri, int32_t i, int32_t j, double b[3], double &q) {
    const int32_t x = kRsOne * i + kRsHalf, y = kRsOne * j + kRsHalf;
    long long E[3];
    const bool in0 = rs_edge(tri.x[1], tri.y[1], tri.x[2], tri.y[2], x, y, E[0]);
    const bool in1 = rs_edge(tri.x[2], tri.y[2], tri.x[0], tri.y[0], x, y, E[1]);
    const bool in2 = rs_edge(tri.x[0], tri.y[0], tri.x[1], tri.y[1], x, y, E[2]);
    if (!(in0 && in1 && in2)) return false;
    const double A = (double)tri.A2;
#pragma unroll
    for (int k = 0; k < 3; ++k) b[k] = (double)E[k] / A;
    q = (b[0] * tri.iz[0] + b[1] * tri.iz[1]) + b[2] * tri.iz[2];
    return true;
}

__device__ inline void rs_draw(const RsTri &tri, uint32_t t, int32_t i, int32_t j, uint32_t W, unsigned long long *zbuf) {
    double b[3], q;
    if (!rs_cover(tri, i, j, b, q)) return;
    const float depth = (float)(1.0 / q);
    const unsigned long long key = ((unsigned long long)__float_as_uint(depth) << 32) | t;
    unsigned long long *cell = zbuf + (size_t)j * W + i;
    // the cell only ever falls: a key that does not beat a value already seen cannot beat the final one
    if (key < __hip_atomic_load(cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(cell, key);
}

// ---- rasterisation ----------------------------------------------------------------------------------------------------------------------------------------

__device__ inline void rs_wave_count(bool mine, uint32_t lane, uint32_t *counter) {
    const unsigned long long m = __ballot(mine);
    if (m && lane == (uint32_t)__ffsll((long long)m) - 1u) atomicAdd(counter, (uint32_t)__popcll(m));
}

__global__ void __launch_bounds__(kRsThreads) k_rs_small(const int32_t *__restrict__ tris, uint32_t T, uint32_t V, const RsRecord *__restrict__ rec, uint32_t H,
                                                         uint32_t W, unsigned long long *zbuf, uint32_t *status, uint32_t *__restrict__ list) {
    const uint32_t t = blockIdx.x * kRsThreads + threadIdx.x, lane = threadIdx.x & 63;
    RsTri tri;
    const RsFate fate = t < T ? rs_setup(tris, t, V, rec, H, W, tri) : kRsNoArea;
    if (fate == kRsBadId) atomicMin(status, t);
    rs_wave_count(fate == kRsNear, lane, status + 1);
    rs_wave_count(fate == kRsGuardBand, lane, status + 2);
    const bool boxed = fate == kRsDraw && tri.i0 <= tri.i1 && tri.j0 <= tri.j1;
    const uint32_t nx = boxed ? (uint32_t)(tri.i1 - tri.i0 + 1) : 0u, ny = boxed ? (uint32_t)(tri.j1 - tri.j0 + 1) : 0u;
    const uint32_t count = nx * ny;                                        // <= 4096^2
    const bool large = count > NSIG_RASTER_SMALL_BOX;
    const unsigned long long m = __ballot(large);
    if (m) {                                                               // (wave-uniform)
        const uint32_t leader = (uint32_t)__ffsll((long long)m) - 1u;
        uint32_t base = 0;
        if (lane == leader) base = atomicAdd(status + 3, (uint32_t)__popcll(m));
        base = __shfl(base, (int)leader, 64);
        if (large) list[base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = t;      // at most T entries: every triangle is listed at most once
    }
    if (large) return;
    for (uint32_t p = 0; p < count; ++p)                                   // at most NSIG_RASTER_SMALL_BOX trips
        rs_draw(tri, t, tri.i0 + (int32_t)(p % nx), tri.j0 + (int32_t)(p / nx), W, zbuf);
}

__global__ void __launch_bounds__(kRsThreads) k_rs_large(const int32_t *__restrict__ tris, uint32_t T, uint32_t V, const RsRecord *__restrict__ rec, uint32_t H,
                                                         uint32_t W, unsigned long long *zbuf, const uint32_t *__restrict__ status, const uint32_t *__restrict__ list) {
    const uint32_t lane = threadIdx.x & 63, wave = (blockIdx.x * kRsThreads + threadIdx.x) >> 6, n_waves = (gridDim.x * kRsThreads) >> 6;
    const uint32_t n = min(status[3], T);                                  // written by k_rs_small, the launch before this one
    for (uint32_t e = wave; e < n; e += n_waves) {
        const uint32_t t = list[e];
        if (t >= T) continue;                                              // (never: k_rs_small lists triangle indices)
        RsTri tri;
        if (rs_setup(tris, t, V, rec, H, W, tri) != kRsDraw || tri.i0 > tri.i1 || tri.j0 > tri.j1) continue;      // (never: it was listed as drawable)
        const uint32_t nx = (uint32_t)(tri.i1 - tri.i0 + 1), count = nx * (uint32_t)(tri.j1 - tri.j0 + 1);
        for (uint32_t p = lane; p < count; p += 64) rs_draw(tri, t, tri.i0 + (int32_t)(p % nx), tri.j0 + (int32_t)(p / nx), W, zbuf);
    }
}

// ---- shading ------------------------------------------------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(kRsThreads) k_rs_shade(const int32_t *__restrict__ tris, uint32_t T, uint32_t V, const RsRecord *__restrict__ rec,
                                                         const float *__restrict__ colors, const float *__restrict__ bg, uint32_t H, uint32_t W,
                                                         const unsigned long long *__restrict__ zbuf, float *__restrict__ image, float *__restrict__ depth,
                                                         int32_t *__restrict__ winner) {
    const uint32_t p = blockIdx.x * kRsThreads + threadIdx.x;
    if (p >= H * W) return;
    float rgb[3] = {bg[0], bg[1], bg[2]}, z = INFINITY;
    int32_t id = -1;
    const unsigned long long cell = zbuf[p];
    const uint32_t t = (uint32_t)cell;
    RsTri tri;
    double b[3], q;
    // a cell rs_raster wrote names a drawable triangle that covers this pixel; anything else (a z-buffer from other arguments) shades as background
    if (cell != kRsEmpty && t < T && rs_setup(tris, t, V, rec, H, W, tri) == kRsDraw && rs_cover(tri, (int32_t)(p % W), (int32_t)(p / W), b, q)) {
        id = (int32_t)t;
        z = __uint_as_float((uint32_t)(cell >> 32));
        double w[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) w[k] = b[k] * tri.iz[k];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const double ca = (double)colors[3 * (size_t)tri.id[0] + ch], cb = (double)colors[3 * (size_t)tri.id[1] + ch], cc = (double)colors[3 * (size_t)tri.id[2] + ch];
            const double n = (w[0] * ca + w[1] * cb) + w[2] * cc;
            rgb[ch] = (float)(n / q);
        }
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) image[3 * (size_t)p + ch] = rgb[ch];
    depth[p] = z;
    winner[p] = id;
}

static int rs_check_sizes(const char *who, uint32_t V, uint32_t T, uint32_t H, uint32_t W) {
    NSIG_REQUIRE(H >= 1 && H <= kRsMaxSide && W >= 1 && W <= kRsMaxSide, "%s: image of %u x %u pixels is out of range (1 .. 4096 each way)", who, H, W);
    NSIG_REQUIRE(V < (1u << 31) && T < (1u << 31), "%s: V=%u, T=%u out of range (each below 2^31)", who, V, T);
    return NSIG_OK;
}

}  // namespace nsig

using namespace nsig;

NSIG_EXPORT size_t rs_scratch_bytes(uint32_t V, uint32_t T, uint32_t H, uint32_t W) {
    if (H < 1 || H > kRsMaxSide || W < 1 || W > kRsMaxSide || V >= (1u << 31) || T >= (1u << 31)) return 0;
    return rs_bytes(V, T, H, W);
}

NSIG_EXPORT int rs_project(const float *vertices, uint32_t V, const float *pose, float fx, float fy, float cx, float cy, float near, uint32_t H, uint32_t W, void *scratch,
                           nsig_stream_t stream) {
    if (int e = rs_check_sizes("rs_project", V, 0, H, W)) return e;
    NSIG_REQUIRE(scratch && pose && (vertices || V == 0), "rs_project: null pointer");
    NSIG_REQUIRE(aligned16(scratch), "rs_project: scratch must be 16-byte aligned");
    const float big = 3.402823466e38f;
    NSIG_REQUIRE(fabsf(fx) <= big && fabsf(fy) <= big && fabsf(cx) <= big && fabsf(cy) <= big, "rs_project: the intrinsics must be finite");
    NSIG_REQUIRE(near > 0.0f && near <= big, "rs_project: the near plane must be a finite number > 0");
    const RsScratch s = rs_split(scratch, V, H, W);
    const uint32_t npix = H * W, n = max(max(V, npix), 4u);
    k_rs_project<<<ceil_div(n, kRsThreads), kRsThreads, 0, as_stream(stream)>>>(vertices, V, pose, fx, fy, cx, cy, near, s.rec, s.zbuf, npix, s.status);
    return check_launch("rs_project");
}

NSIG_EXPORT int rs_raster(const int32_t *triangles, uint32_t T, uint32_t V, uint32_t H, uint32_t W, void *scratch, nsig_stream_t stream) {
    if (int e = rs_check_sizes("rs_raster", V, T, H, W)) return e;
    NSIG_REQUIRE(scratch && (triangles || T == 0), "rs_raster: null pointer");
    NSIG_REQUIRE(aligned16(scratch), "rs_raster: scratch must be 16-byte aligned");
    if (T == 0 || V == 0) return NSIG_OK;
    const RsScratch s = rs_split(scratch, V, H, W);
    k_rs_small<<<ceil_div(T, kRsThreads), kRsThreads, 0, as_stream(stream)>>>(triangles, T, V, s.rec, H, W, s.zbuf, s.status, s.list);
    k_rs_large<<<kRsLargeBlocks, kRsThreads, 0, as_stream(stream)>>>(triangles, T, V, s.rec, H, W, s.zbuf, s.status, s.list);
    return check_launch("rs_raster");
}

NSIG_EXPORT int rs_shade(const int32_t *triangles, uint32_t T, uint32_t V, const float *colors, const float *bg, uint32_t H, uint32_t W, const void *scratch, float *image,
                         float *depth, int32_t *triangle, nsig_stream_t stream) {
    if (int e = rs_check_sizes("rs_shade", V, T, H, W)) return e;
    NSIG_REQUIRE(scratch && bg && image && depth && triangle && (triangles || T == 0) && (colors || V == 0), "rs_shade: null pointer");
    NSIG_REQUIRE(aligned16(scratch), "rs_shade: scratch must be 16-byte aligned");
    const RsScratch s = rs_split(const_cast<void *>(scratch), V, H, W);
    k_rs_shade<<<ceil_div(H * W, kRsThreads), kRsThreads, 0, as_stream(stream)>>>(triangles, T, V, s.rec, colors, bg, H, W, s.zbuf, image, depth, triangle);
    return check_launch("rs_shade");
}
