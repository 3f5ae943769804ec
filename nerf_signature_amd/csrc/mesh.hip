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
    NSIG_REQUIRE(reinterpret_cast<uintptr_t>(scratch) % 16 == 0, "mc_count: scratch must be 16-byte aligned");
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
    NSIG_REQUIRE(reinterpret_cast<uintptr_t>(scratch) % 16 == 0, "mc_emit: scratch must be 16-byte aligned");
    NSIG_REQUIRE((n_vertices == 0) == (n_triangles == 0), "mc_emit: %u vertices with %u triangles: not the totals of mc_count", n_vertices, n_triangles);
    if (n_vertices == 0) return NSIG_OK;
    NSIG_REQUIRE(vertices && triangles, "mc_emit: null pointer");
    const McDims d = make_dims(nx, ny, nz);
    const McScratch s = mc_split(scratch, d.N);
    k_mc_verts<<<s.nb, kMcThreads, 0, as_stream(stream)>>>(u, d, threshold, s.code, s.sums, s.vbase, vertices);
    k_mc_tris<<<s.nb, kMcThreads, 0, as_stream(stream)>>>(d, s.code, s.sums + s.nb, s.vbase, triangles);
    return check_launch("mc_emit");
}
