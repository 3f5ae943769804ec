// Marching cubes over a dense fp32 lattice (replaces the reference's mcubes.marching_cubes call in extract_geometry, nerf/utils.py:192-204).
//
// u[nx, ny, nz] is row-major with z fastest.  Node n = (i ny + j) nz + k is inside when u[n] > threshold (NaN is outside).  Node n owns its
// +x, +y and +z edges where they exist, and is the min corner of a cell when i < nx-1, j < ny-1, k < nz-1.  Output order (fully determined):
//   vertices: by node in C order, then by axis x, y, z, one per crossing edge, in lattice space -- the node's integer coordinates with the
//             crossing axis replaced by float(i) + t, t = (threshold - a) / (b - a) clamped to [0, 1] (NaN -> 0.5);
//   triangles: by cell in C order, then in table order (mc_tables.h); int32 triples of vertex ids.
// Four launches: count (per-node case + edge bits, per-block totals) -> scan of the block totals (one workgroup) -> vertex emit (per-node
// vertex base, in-block ballot offsets) -> triangle emit (ids through the vertex bases of the nodes that own the cell's edges).
#include "wave.h"
#include "mc_tables.h"

namespace nsig {

constexpr uint32_t kMcThreads = 256;                  // 4 waves
constexpr uint32_t kMcRounds = 4;
constexpr uint32_t kMcNodes = kMcThreads * kMcRounds;  // nodes per workgroup: node base + 256 r + tid in round r (coalesced, C order by round)
constexpr uint64_t kMcMaxNodes = 1ull << 28;

struct McDims {
    uint32_t nx, ny, nz, N, sx, sy;   // sx = ny nz, sy = nz
};

static inline size_t align256(size_t b) { return (b + 255) & ~size_t(255); }

// scratch: code[N] uint16 (case | edge bits << 8), vbase[N] uint32, sums[2 nb] uint32 (vertex then triangle totals per workgroup -> their
// exclusive prefix sums after the scan)
struct McScratch {
    uint16_t *code;
    uint32_t *vbase, *sums;
    uint32_t nb;
};
static inline size_t mc_bytes(uint32_t N) {
    const uint32_t nb = ceil_div(N, kMcNodes);
    return align256(size_t(N) * 2) + align256(size_t(N) * 4) + align256(size_t(nb) * 8);
}
static inline McScratch mc_split(void *scratch, uint32_t N) {
    char *p = static_cast<char *>(scratch);
    McScratch s;
    s.nb = ceil_div(N, kMcNodes);
    s.code = reinterpret_cast<uint16_t *>(p);
    s.vbase = reinterpret_cast<uint32_t *>(p + align256(size_t(N) * 2));
    s.sums = reinterpret_cast<uint32_t *>(p + align256(size_t(N) * 2) + align256(size_t(N) * 4));
    return s;
}

__device__ inline uint32_t lanes_below(unsigned long long m, uint32_t lane) { return (uint32_t)__popcll(m & ((1ull << lane) - 1ull)); }

// Exclusive prefix of a small per-lane count (< 2^bits) inside the wave, and the wave's total: one ballot per bit.
template <int Bits>
__device__ inline uint32_t wave_prefix(uint32_t c, uint32_t lane, uint32_t &total) {
    uint32_t pre = 0;
    total = 0;
#pragma unroll
    for (int b = 0; b < Bits; ++b) {
        const unsigned long long m = __ballot((c >> b) & 1u);
        pre += lanes_below(m, lane) << b;
        total += (uint32_t)__popcll(m) << b;
    }
    return pre;
}

// Pass 1: per node the case of the cell it is the min corner of (0 where there is no cell) and the crossing bits of its owned edges;
// per workgroup the vertex and triangle totals.
__global__ void __launch_bounds__(kMcThreads) k_mc_count(const float *__restrict__ u, McDims d, float thr, uint16_t *__restrict__ code,
                                                         uint32_t *__restrict__ sums, uint32_t nb) {
    __shared__ uint32_t red[2][kMcThreads / kWave];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    uint32_t nv = 0, nt = 0;
#pragma unroll
    for (uint32_t r = 0; r < kMcRounds; ++r) {
        const uint32_t n = blockIdx.x * kMcNodes + r * kMcThreads + tid;
        if (n >= d.N) continue;
        const uint32_t k = n % d.nz, jk = n / d.nz, j = jk % d.ny, i = jk / d.ny;
        const bool hx = i + 1 < d.nx, hy = j + 1 < d.ny, hz = k + 1 < d.nz;
        const bool c0 = u[n] > thr;
        const bool cx = hx && u[n + d.sx] > thr, cy = hy && u[n + d.sy] > thr, cz = hz && u[n + 1] > thr;
        const uint32_t bits = (hx && cx != c0 ? 1u : 0u) | (hy && cy != c0 ? 2u : 0u) | (hz && cz != c0 ? 4u : 0u);
        uint32_t cas = 0;
        if (hx && hy && hz) {
            const bool cxy = u[n + d.sx + d.sy] > thr, cxz = u[n + d.sx + 1] > thr, cyz = u[n + d.sy + 1] > thr, cxyz = u[n + d.sx + d.sy + 1] > thr;
            cas = (uint32_t)c0 | (uint32_t)cx << 1 | (uint32_t)cy << 2 | (uint32_t)cxy << 3 | (uint32_t)cz << 4 | (uint32_t)cxz << 5 |
                  (uint32_t)cyz << 6 | (uint32_t)cxyz << 7;
        }
        code[n] = (uint16_t)(cas | bits << 8);
        nv += (uint32_t)__popc(bits);
        nt += mc_tri_count[cas];
    }
    nv = wave_sum(nv);
    nt = wave_sum(nt);
    if (lane == 0) {
        red[0][wid] = nv;
        red[1][wid] = nt;
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t a = 0, b = 0;
#pragma unroll
        for (uint32_t w = 0; w < kMcThreads / kWave; ++w) {
            a += red[0][w];
            b += red[1][w];
        }
        sums[blockIdx.x] = a;
        sums[nb + blockIdx.x] = b;
    }
}

// Pass 2: exclusive prefix sums of the 2 nb workgroup totals, in place; totals[0] = V, totals[1] = T.  One 1024-thread workgroup, each
// thread a contiguous run of entries, the runs' sums through block_exclusive_sum (as k_march_scan), one array after the other.
__global__ void __launch_bounds__(1024) k_mc_scan(uint32_t *__restrict__ sums, uint32_t nb, uint32_t *__restrict__ totals) {
    __shared__ uint32_t wave_tot[16];
    const uint32_t tid = threadIdx.x;
    const uint32_t chunk = ceil_div(nb, 1024u);
    const uint32_t beg = min(nb, tid * chunk), end = min(nb, beg + chunk);
    for (uint32_t a = 0; a < 2; ++a) {
        uint32_t *s = sums + size_t(a) * nb;
        uint32_t sum = 0;
        for (uint32_t i = beg; i < end; ++i) sum += s[i];
        uint32_t total;
        uint32_t off = block_exclusive_sum<16>(sum, wave_tot, &total);
        for (uint32_t i = beg; i < end; ++i) {
            const uint32_t c = s[i];
            s[i] = off;
            off += c;
        }
        if (tid == 0) totals[a] = total;
        __syncthreads();
    }
}

// Pass 3: every node's vertex base, and the vertices of its crossing edges.
__global__ void __launch_bounds__(kMcThreads) k_mc_verts(const float *__restrict__ u, McDims d, float thr, const uint16_t *__restrict__ code,
                                                         const uint32_t *__restrict__ voff, uint32_t *__restrict__ vbase, float *__restrict__ verts) {
    __shared__ uint32_t wave_cnt[kMcThreads / kWave];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    uint32_t running = voff[blockIdx.x];
#pragma unroll
    for (uint32_t r = 0; r < kMcRounds; ++r) {
        const uint32_t n = blockIdx.x * kMcNodes + r * kMcThreads + tid;
        const uint32_t bits = n < d.N ? (uint32_t)(code[n] >> 8) : 0u;
        uint32_t wtot;
        const uint32_t pre = wave_prefix<2>((uint32_t)__popc(bits), lane, wtot);
        if (lane == 0) wave_cnt[wid] = wtot;
        __syncthreads();
        uint32_t off = running, round_total = 0;
#pragma unroll
        for (uint32_t w = 0; w < kMcThreads / kWave; ++w) {
            const uint32_t c = wave_cnt[w];
            if (w < wid) off += c;
            round_total += c;
        }
        off += pre;
        if (n < d.N) {
            vbase[n] = off;
            if (bits) {
                const uint32_t k = n % d.nz, jk = n / d.nz, j = jk % d.ny, i = jk / d.ny;
                const float a = u[n];
                const uint32_t step[3] = {d.sx, d.sy, 1u};
#pragma unroll
                for (uint32_t ax = 0; ax < 3; ++ax) {
                    if (!((bits >> ax) & 1u)) continue;
                    const float b = u[n + step[ax]];
                    float t = (thr - a) / (b - a);
                    t = isnan(t) ? 0.5f : fminf(fmaxf(t, 0.0f), 1.0f);
                    float p[3] = {(float)i, (float)j, (float)k};
                    p[ax] = p[ax] + t;
                    float *o = verts + 3 * (size_t)off;
                    o[0] = p[0];
                    o[1] = p[1];
                    o[2] = p[2];
                    ++off;
                }
            }
        }
        running += round_total;
        __syncthreads();
    }
}

// Pass 4: every cell's triangles; an edge's vertex id is its owner node's vertex base plus the owner's crossing edges of lower axis.
__global__ void __launch_bounds__(kMcThreads) k_mc_tris(McDims d, const uint16_t *__restrict__ code, const uint32_t *__restrict__ toff,
                                                        const uint32_t *__restrict__ vbase, int32_t *__restrict__ tris) {
    __shared__ uint32_t wave_cnt[kMcThreads / kWave];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    uint32_t running = toff[blockIdx.x];
    const uint32_t corner_off[8] = {0u, d.sx, d.sy, d.sx + d.sy, 1u, d.sx + 1u, d.sy + 1u, d.sx + d.sy + 1u};
#pragma unroll
    for (uint32_t r = 0; r < kMcRounds; ++r) {
        const uint32_t n = blockIdx.x * kMcNodes + r * kMcThreads + tid;
        const uint32_t cas = n < d.N ? (uint32_t)(code[n] & 0xffu) : 0u;
        const uint32_t cnt = mc_tri_count[cas];
        uint32_t wtot;
        const uint32_t pre = wave_prefix<3>(cnt, lane, wtot);
        if (lane == 0) wave_cnt[wid] = wtot;
        __syncthreads();
        uint32_t off = running, round_total = 0;
#pragma unroll
        for (uint32_t w = 0; w < kMcThreads / kWave; ++w) {
            const uint32_t c = wave_cnt[w];
            if (w < wid) off += c;
            round_total += c;
        }
        off += pre;
        for (uint32_t t = 0; t < cnt; ++t) {
            int32_t *o = tris + 3 * (size_t)(off + t);
#pragma unroll
            for (uint32_t v = 0; v < 3; ++v) {
                const int e = mc_tri_edges[cas][3 * t + v];
                const uint32_t owner = n + corner_off[mc_edge_corner[e]], ax = (uint32_t)mc_edge_axis[e];
                const uint32_t below = (uint32_t)(code[owner] >> 8) & ((1u << ax) - 1u);
                o[v] = (int32_t)(vbase[owner] + (uint32_t)__popc(below));
            }
        }
        running += round_total;
        __syncthreads();
    }
}

// ---- vertex normals -------------------------------------------------------------------------------------------------------------------------------------
// Finite-difference gradient of u at a node along one axis of extent ext (>= 2): central inside, one-sided at the two ends.
__device__ inline float mc_diff(const float *__restrict__ u, uint32_t n, uint32_t i, uint32_t ext, uint32_t stride) {
    if (i == 0) return u[n + stride] - u[n];
    if (i == ext - 1) return u[n] - u[n - stride];
    return (u[n + stride] - u[n - stride]) * 0.5f;
}

__device__ inline void mc_node_grad(const float *__restrict__ u, const McDims &d, uint32_t n, uint32_t i, uint32_t j, uint32_t k, float g[3]) {
    g[0] = mc_diff(u, n, i, d.nx, d.sx);
    g[1] = mc_diff(u, n, j, d.ny, d.sy);
    g[2] = mc_diff(u, n, k, d.nz, 1u);
}

// One thread per node, after mc_emit: for every crossing edge the node owns, the normal of the vertex k_mc_verts wrote for it, to the same index
// (vbase[n] + the node's crossing edges of lower axis).  The gradient is interpolated between the edge's two nodes at k_mc_verts' own t, scaled per
// axis, and the normal is its negated unit vector (density grows inwards); a zero or non-finite length gives (0, 0, 0).  grads (optional) receives
// the scaled gradient before the division.
__global__ void __launch_bounds__(kMcThreads) k_mc_normals(const float *__restrict__ u, McDims d, float thr, const uint16_t *__restrict__ code,
                                                           const uint32_t *__restrict__ vbase, uint32_t n_vertices, float sx, float sy, float sz,
                                                           float *__restrict__ normals, float *__restrict__ grads) {
    const uint32_t n = blockIdx.x * kMcThreads + threadIdx.x;
    if (n >= d.N) return;
    const uint32_t bits = (uint32_t)(code[n] >> 8);
    if (!bits) return;
    const uint32_t k = n % d.nz, jk = n / d.nz, j = jk % d.ny, i = jk / d.ny;
    const float a = u[n];
    float ga[3];
    mc_node_grad(u, d, n, i, j, k, ga);
    const uint32_t step[3] = {d.sx, d.sy, 1u};
    const float scale[3] = {sx, sy, sz};
    uint32_t off = vbase[n];
#pragma unroll
    for (uint32_t ax = 0; ax < 3; ++ax) {
        if (!((bits >> ax) & 1u)) continue;
        if (!(ax == 0 ? i + 1 < d.nx : ax == 1 ? j + 1 < d.ny : k + 1 < d.nz)) continue;      // (never, with mc_count's codes: a crossing edge has its far node)
        const uint32_t m = n + step[ax];
        const float b = u[m];
        float t = (thr - a) / (b - a);
        t = isnan(t) ? 0.5f : fminf(fmaxf(t, 0.0f), 1.0f);
        float gb[3];
        mc_node_grad(u, d, m, i + (ax == 0), j + (ax == 1), k + (ax == 2), gb);
        float g[3];
#pragma unroll
        for (uint32_t c = 0; c < 3; ++c) g[c] = (ga[c] + t * (gb[c] - ga[c])) * scale[c];
        const float len = sqrtf((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
        const bool ok = len > 0.0f && len < INFINITY;      // false for NaN too
        if (off < n_vertices) {                             // (always, with the scratch mc_emit left for these very arguments)
            float *o = normals + 3 * (size_t)off;
#pragma unroll
            for (uint32_t c = 0; c < 3; ++c) o[c] = ok ? -g[c] / len : 0.0f;
            if (grads) {
                float *q = grads + 3 * (size_t)off;
#pragma unroll
                for (uint32_t c = 0; c < 3; ++c) q[c] = g[c];
            }
        }
        ++off;
    }
}

// ---- connected components of a triangle mesh ----------------------------------------------------------------------------------------------------------
// A union-find forest in labels[] itself: labels[v] is v's parent.  Invariant, from the first store to the last: labels[v] <= v, and a
// vertex whose parent is not itself never becomes a root again.  Hence every pointer walk strictly descends and ends within v steps whatever other
// threads do, no cycle can form, and a tree's root is its smallest id.  Roots are hooked by compare-and-swap (larger root under the smaller); path
// halving only ever lowers a parent to one of its own ancestors.  No thread waits for another: a failed compare-and-swap means another thread hooked
// that root, and the retry goes on from a strictly smaller pair of ids.  Every shared word is read and written with agent-scope atomics.
constexpr uint32_t kCcThreads = 256;
constexpr uint32_t kCcNoError = 0xffffffffu;
constexpr size_t kCcScratchBytes = 256;      // word 0: kCcNoError, or the index of the first triangle with an id outside [0, V)

__device__ inline int32_t cc_load(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Root of x's tree, halving the path on the way (each parent lowered to the grandparent read just before: an ancestor, smaller than the parent).
__device__ inline int32_t cc_find(int32_t *parent, int32_t x) {
    int32_t px = cc_load(parent + x);
    while (px != x) {                      // px < x
        const int32_t g = cc_load(parent + px);
        if (g != px) atomicMin(parent + x, g);
        x = px;
        px = g;
    }
    return x;
}

// The same walk without a store (the flatten pass: every root is final).
__device__ inline int32_t cc_root(const int32_t *parent, int32_t x) {
    int32_t px = cc_load(parent + x);
    while (px != x) {
        x = px;
        px = cc_load(parent + x);
    }
    return x;
}

// Join the trees of a and b.  a + b falls with every failed compare-and-swap, so the loop ends on its own.
__device__ inline void cc_hook(int32_t *parent, int32_t a, int32_t b) {
    a = cc_find(parent, a);
    b = cc_find(parent, b);
    while (a != b) {
        const int32_t hi = max(a, b), lo = min(a, b);
        const int32_t old = atomicCAS(parent + hi, hi, lo);
        if (old == hi) break;              // hi was a root and now hangs under lo < hi
        a = cc_find(parent, old);          // another thread hooked hi under old < hi: go on from there
        b = lo;
    }
}

__global__ void __launch_bounds__(kCcThreads) k_cc_init(int32_t *__restrict__ labels, uint32_t V, uint32_t *__restrict__ err) {
    const uint32_t v = blockIdx.x * kCcThreads + threadIdx.x;
    if (v == 0) *err = kCcNoError;
    if (v < V) labels[v] = (int32_t)v;
}

__global__ void __launch_bounds__(kCcThreads) k_cc_hook(const int32_t *__restrict__ tris, uint32_t T, uint32_t V, int32_t *labels, uint32_t *err) {
    const uint32_t t = blockIdx.x * kCcThreads + threadIdx.x;
    if (t >= T) return;
    const int32_t a = tris[3 * (size_t)t], b = tris[3 * (size_t)t + 1], c = tris[3 * (size_t)t + 2];
    if ((uint32_t)a >= V || (uint32_t)b >= V || (uint32_t)c >= V) {      // (negative ids wrap above 2^31 > V)
        atomicMin(err, t);
        return;
    }
    cc_hook(labels, a, b);                 // two sides connect the three corners; the third adds nothing
    cc_hook(labels, b, c);
}

__global__ void __launch_bounds__(kCcThreads) k_cc_flatten(int32_t *labels, uint32_t V) {
    const uint32_t v = blockIdx.x * kCcThreads + threadIdx.x;
    if (v >= V) return;
    const int32_t r = cc_root(labels, (int32_t)v);
    __hip_atomic_store(labels + v, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // r <= every value labels[v] has held: walks through v stay valid
}

static int check_dims(const char *what, uint32_t nx, uint32_t ny, uint32_t nz) {
    NSIG_REQUIRE(nx >= 2 && ny >= 2 && nz >= 2, "%s: every lattice dimension must be at least 2 (got %u x %u x %u)", what, nx, ny, nz);
    NSIG_REQUIRE((uint64_t)nx * ny * nz <= kMcMaxNodes, "%s: lattice of %u x %u x %u nodes is out of range (at most 2^28 nodes)", what, nx, ny, nz);
    return NSIG_OK;
}

static McDims make_dims(uint32_t nx, uint32_t ny, uint32_t nz) { return McDims{nx, ny, nz, nx * ny * nz, ny * nz, nz}; }

}  // namespace nsig

using namespace nsig;

NSIG_EXPORT size_t mc_scratch_bytes(uint32_t nx, uint32_t ny, uint32_t nz) {
    if (nx < 2 || ny < 2 || nz < 2 || (uint64_t)nx * ny * nz > kMcMaxNodes) return 0;
    return mc_bytes(nx * ny * nz);
}

NSIG_EXPORT int mc_count(const float *u, uint32_t nx, uint32_t ny, uint32_t nz, float threshold, void *scratch, uint32_t *totals, nsig_stream_t stream) {
    NSIG_REQUIRE(u && scratch && totals, "mc_count: null pointer");
    if (int e = check_dims("mc_count", nx, ny, nz)) return e;
    NSIG_REQUIRE(aligned16(scratch), "mc_count: scratch must be 16-byte aligned");
    const McDims d = make_dims(nx, ny, nz);
    const McScratch s = mc_split(scratch, d.N);
    k_mc_count<<<s.nb, kMcThreads, 0, as_stream(stream)>>>(u, d, threshold, s.code, s.sums, s.nb);
    k_mc_scan<<<1, 1024, 0, as_stream(stream)>>>(s.sums, s.nb, totals);
    return check_launch("mc_count");
}

NSIG_EXPORT int mc_emit(const float *u, uint32_t nx, uint32_t ny, uint32_t nz, float threshold, void *scratch, uint32_t n_vertices, uint32_t n_triangles,
                        float *vertices, int32_t *triangles, nsig_stream_t stream) {
    NSIG_REQUIRE(u && scratch, "mc_emit: null pointer");
    if (int e = check_dims("mc_emit", nx, ny, nz)) return e;
    NSIG_REQUIRE(aligned16(scratch), "mc_emit: scratch must be 16-byte aligned");
    NSIG_REQUIRE((n_vertices == 0) == (n_triangles == 0), "mc_emit: %u vertices with %u triangles: not the totals of mc_count", n_vertices, n_triangles);
    if (n_vertices == 0) return NSIG_OK;
    NSIG_REQUIRE(vertices && triangles, "mc_emit: null pointer");
    const McDims d = make_dims(nx, ny, nz);
    const McScratch s = mc_split(scratch, d.N);
    k_mc_verts<<<s.nb, kMcThreads, 0, as_stream(stream)>>>(u, d, threshold, s.code, s.sums, s.vbase, vertices);
    k_mc_tris<<<s.nb, kMcThreads, 0, as_stream(stream)>>>(d, s.code, s.sums + s.nb, s.vbase, triangles);
    return check_launch("mc_emit");
}

NSIG_EXPORT int mc_vertex_normals(const float *u, uint32_t nx, uint32_t ny, uint32_t nz, float threshold, const void *scratch, uint32_t n_vertices,
                                  float scale_x, float scale_y, float scale_z, float *normals, float *gradients, nsig_stream_t stream) {
    NSIG_REQUIRE(u && scratch, "mc_vertex_normals: null pointer");
    if (int e = check_dims("mc_vertex_normals", nx, ny, nz)) return e;
    NSIG_REQUIRE(aligned16(scratch), "mc_vertex_normals: scratch must be 16-byte aligned");
    NSIG_REQUIRE((uint64_t)n_vertices <= 3ull * nx * ny * nz, "mc_vertex_normals: %u vertices is out of range for %u x %u x %u nodes", n_vertices, nx, ny, nz);
    if (n_vertices == 0) return NSIG_OK;
    NSIG_REQUIRE(normals, "mc_vertex_normals: null pointer");
    const McDims d = make_dims(nx, ny, nz);
    const McScratch s = mc_split(const_cast<void *>(scratch), d.N);
    k_mc_normals<<<ceil_div(d.N, kMcThreads), kMcThreads, 0, as_stream(stream)>>>(u, d, threshold, s.code, s.vbase, n_vertices, scale_x, scale_y, scale_z, normals,
                                                                                  gradients);
    return check_launch("mc_vertex_normals");
}

NSIG_EXPORT size_t mesh_components_scratch_bytes(uint32_t V, uint32_t T) {
    if (V >= (1u << 31) || T >= (1u << 31)) return 0;
    return kCcScratchBytes;
}

NSIG_EXPORT int mesh_components(const int32_t *triangles, uint32_t T, uint32_t V, int32_t *labels, void *scratch, nsig_stream_t stream) {
    NSIG_REQUIRE(V < (1u << 31) && T < (1u << 31), "mesh_components: V=%u, T=%u out of range (each below 2^31)", V, T);
    NSIG_REQUIRE(scratch && (triangles || T == 0) && (labels || V == 0), "mesh_components: null pointer");
    NSIG_REQUIRE(aligned16(scratch), "mesh_components: scratch must be 16-byte aligned");
    uint32_t *err = static_cast<uint32_t *>(scratch);
    k_cc_init<<<max(1u, ceil_div(V, kCcThreads)), kCcThreads, 0, as_stream(stream)>>>(labels, V, err);
    if (T) k_cc_hook<<<ceil_div(T, kCcThreads), kCcThreads, 0, as_stream(stream)>>>(triangles, T, V, labels, err);
    if (T && V) k_cc_flatten<<<ceil_div(V, kCcThreads), kCcThreads, 0, as_stream(stream)>>>(labels, V);
    return check_launch("mesh_components");
}
