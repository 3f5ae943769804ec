// Hash-grid kernels for gfx950: codebook pre-sum, stand-alone encoders, codebook backward scatter,
// gradient fan-out.  Behavioural references: /root/reference/hash_encoding.py:96-111 (base encoder),
// /root/reference/hash_encoding_wtmk_bit.py:99-116 (codebook encoder) and their autograd.
//
// Two algebraic facts of the reference drive the design (both verified against the reference itself in
// tests/test_oracle_golden.py):
//   (1) all D codebook levels have the same resolution (2048) and hash, hence identical corner rows and
//       weights, and the encoder output is the SUM of the D interpolations.  Interpolation is linear in
//       the table, so  sum_i lerp(table_i) == lerp(sum_i table_i):  one streaming pass builds
//       S = sum_i table_{2i+bit_i}  (D x 4 MiB read, 4 MiB written) and every point then needs ONE
//       8-corner gather in S instead of D of them;
//   (2) for the same reason every selected table receives the SAME gradient G[T,2]; the backward
//       scatters once into G and a fan-out pass copies G into the D gradient tensors autograd expects.
#include <cstdlib>
#include "adam.h"
#include "hashgrid.h"
#include "wave.h"

namespace nsig {

// S[e] = sum_i tables[i][e]; float4 per lane (1 KiB per wave-instruction), D independent streams.
__global__ void __launch_bounds__(256) k_codebook_presum(CodebookPtrs tabs, uint32_t D, float4 *__restrict__ S) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;  // float4 index, T*2/4 of them
    if (e >= NSIG_TABLE_ROWS / 2) return;
    float4 acc = {0.f, 0.f, 0.f, 0.f};
    uint32_t i = 0;
    for (; i + 4 <= D; i += 4) {  // four loads in flight per lane
        const float4 a = reinterpret_cast<const float4 *>(tabs.p[i])[e];
        const float4 b = reinterpret_cast<const float4 *>(tabs.p[i + 1])[e];
        const float4 c = reinterpret_cast<const float4 *>(tabs.p[i + 2])[e];
        const float4 d = reinterpret_cast<const float4 *>(tabs.p[i + 3])[e];
        acc.x = (((acc.x + a.x) + b.x) + c.x) + d.x;
        acc.y = (((acc.y + a.y) + b.y) + c.y) + d.y;
        acc.z = (((acc.z + a.z) + b.z) + c.z) + d.z;
        acc.w = (((acc.w + a.w) + b.w) + c.w) + d.w;
    }
    for (; i < D; ++i) {
        const float4 a = reinterpret_cast<const float4 *>(tabs.p[i])[e];
        acc.x += a.x; acc.y += a.y; acc.z += a.z; acc.w += a.w;
    }
    S[e] = acc;
}

// Stand-alone base encoder (+ optional codebook via S): one lane per (point, level); a wave covers
// 4 points x 16 levels and stores 4 full 128-byte feature rows.
__global__ void __launch_bounds__(256) k_encode(const float *__restrict__ x01, uint32_t M, TablePtrs base, LevelGeom geom,
                                                const float *__restrict__ S, float *__restrict__ feat) {
    const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t m = gid >> 4, l = gid & 15u;
    if (m >= M) return;
    const float x = x01[3 * (size_t)m], y = x01[3 * (size_t)m + 1], z = x01[3 * (size_t)m + 2];
    float2 f = encode_level(base.p[l], x, y, z, geom.cell[l]);
    if (S != nullptr && l == 15u) {  // network_wtmk_tcnn.py:106: codebook feature added into channels 30:32
        const float2 c = encode_level(S, x, y, z, geom.cell[NSIG_BASE_LEVELS]);
        f.x = f.x + c.x;
        f.y = f.y + c.y;
    }
    reinterpret_cast<float2 *>(feat)[(size_t)m * 16 + l] = f;
}

// The codebook encoder evaluated literally (D gathers per corner, summed in bit order).
__global__ void __launch_bounds__(256) k_codebook_encode(const float *__restrict__ x01, uint32_t M, CodebookPtrs tabs, uint32_t D,
                                                         float cell, float *__restrict__ out) {
    const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    Corner8 c;
    corner_rows(x01[3 * (size_t)m], x01[3 * (size_t)m + 1], x01[3 * (size_t)m + 2], cell, c);
    float2 acc = {0.f, 0.f};
    for (uint32_t i = 0; i < D; ++i) {
        float2 e[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) e[k] = reinterpret_cast<const float2 *>(tabs.p[i])[c.row[k]];
        const float2 v = trilerp(e, c.wx, c.wy, c.wz);
        acc.x += v.x;
        acc.y += v.y;
    }
    reinterpret_cast<float2 *>(out)[m] = acc;
}

// G[row_k] += w_k * dfeat for the 8 corners of every point: 16 lanes per point, lane = (corner, feature),
// so the two features of a row are adjacent lanes (one 8-byte segment per pair of lanes).
__global__ void __launch_bounds__(256) k_codebook_bwd(const float *__restrict__ x01, uint32_t M, const float *__restrict__ dfeat,
                                                      float cell, float *__restrict__ G) {
    const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t m = gid >> 4, k = (gid >> 1) & 7u, f = gid & 1u;
    if (m >= M) return;
    const float g = dfeat[2 * (size_t)m + f];
    if (g == 0.0f) return;  // padded rows and rays past early termination carry exact zeros
    Corner8 c;
    corner_rows(x01[3 * (size_t)m], x01[3 * (size_t)m + 1], x01[3 * (size_t)m + 2], cell, c);
    atomicAdd(G + 2 * (size_t)c.row[k] + f, corner_weight(c, (int)k, g));
}

// Owner-computes scatter.  Memory-side float atomics retire ~2e10 requests/s chip-wide however they are spread
// (MI355X_MICROARCH.md, Global float atomics), and the point-wise scatter needs >= 4 requests per point; LDS
// atomics and a contiguous flush need 1/10 of that.  Workgroup (slice s, replica r) owns rows [s*16384, (s+1)*16384)
// of G in LDS, scans points [r*M/8, (r+1)*M/8) and keeps only the corners whose row falls in its slice (the hash
// makes that 1 corner in 32, so every workgroup tests every point: 32x redundant work, cheap next to the atomics it
// replaces -- and kept cheap: the record carries the integer cell and the weights, computed once by k_field_bwd).
// blockIdx = s*8 + r, so the 32 workgroups that scan the same points share one XCD (blockIdx % 8) and its L2 serves the
// re-reads.  Phase stamps (tools/scatter_timing.py): 1.4 us zeroing, the scan, 6 us flush; the scan was a chain of exposed L2
// latencies (one record in flight per thread) until four were prefetched.  Tried and rejected: collecting hits in a bit mask or
// in a per-wave LDS ring to run the weight/atomic code with full lanes -- both slower than the plain predicated body.
constexpr int kSliceRows = 16384, kSlices = NSIG_TABLE_ROWS / kSliceRows, kReplicas = 8;

#ifdef NSIG_DEC_TIMING
__device__ unsigned long long g_scatter_stamps[8];
#define SC_STAMP(k)                                                                      \
    do {                                                                                 \
        __builtin_amdgcn_sched_barrier(0);                                               \
        if (blockIdx.x == 0 && threadIdx.x == 0) g_scatter_stamps[k] = wall_clock64();   \
        __builtin_amdgcn_sched_barrier(0);                                               \
    } while (0)
#else
#define SC_STAMP(k)
#endif

// `sets` record arrays of M points each (one for the codebook; 16, one per base level, in stage-1 training), each scattered into
// its own table.  replicas == 1: every row has one owner, which stores.  Workgroup order for sets = 16: rounds of 8 sets, set =
// 8*round + blockIdx % 8, so the 32*replicas workgroups that scan one set's records share an XCD (blockIdx % 8) whose L2 holds
// that one record array (4 MiB at 131 k points); interleaving all 16 sets put two arrays on every XCD and doubled the time.
struct ScatterTargets {
    float *g[NSIG_BASE_LEVELS];
};
__global__ void __launch_bounds__(1024) k_scatter_sliced(const float *__restrict__ rec_all, uint32_t M, ScatterTargets tg, uint32_t sets, uint32_t replicas) {
    extern __shared__ float acc[];  // [kSliceRows][2]
    uint32_t set = 0, sr = blockIdx.x;
    if (sets > 1) {
        const uint32_t per_round = 8u * kSlices * replicas, round = blockIdx.x / per_round, b = blockIdx.x - round * per_round;
        set = round * 8u + (b & 7u);
        sr = b >> 3;
        if (set >= sets) return;
    }
    const uint32_t slice = sr / replicas, replica = sr - slice * replicas;
    const float *__restrict__ rec = rec_all + (size_t)set * M * 8;
    float *__restrict__ G = tg.g[set];
    const uint32_t kReplicasRt = replicas;
    SC_STAMP(0);
    for (uint32_t i = threadIdx.x; i < 2u * kSliceRows; i += blockDim.x) acc[i] = 0.0f;
    __syncthreads();
    SC_STAMP(1);
    const uint32_t chunk = ceil_div(M, kReplicasRt);
    const uint32_t beg = min(M, replica * chunk), end = min(M, beg + chunk);
    const uint4 *__restrict__ rec4 = reinterpret_cast<const uint4 *>(rec);
    // With 16 waves per CU and ~150 points per thread the scan is a chain of exposed L2 latencies unless several points'
    // records are in flight per thread: four at a time.
    constexpr int kAhead = 4;
    for (uint32_t m0 = beg + threadIdx.x; m0 < end; m0 += blockDim.x * kAhead) {
        uint4 ra[kAhead], rb[kAhead];
#pragma unroll
        for (int u = 0; u < kAhead; ++u) {
            const uint32_t m = min(m0 + u * blockDim.x, end - 1);   // clamped: the duplicate is skipped below
            ra[u] = rec4[2 * (size_t)m];
            rb[u] = rec4[2 * (size_t)m + 1];
        }
#pragma unroll
        for (int u = 0; u < kAhead; ++u) {
            if (m0 + u * blockDim.x >= end) break;
            const float g0 = __uint_as_float(rb[u].y), g1 = __uint_as_float(rb[u].z);
            if (g0 == 0.0f && g1 == 0.0f) continue;  // padding rows and terminated rays
            Corner8 c;
            c.wx = __uint_as_float(ra[u].z); c.wy = __uint_as_float(ra[u].w); c.wz = __uint_as_float(rb[u].x);
            const uint32_t ix = ra[u].x & 0xffffu, iy = ra[u].x >> 16, iz = ra[u].y;
            const uint32_t hy[2] = {iy * kPrimeY, (iy + 1u) * kPrimeY};
            const uint32_t hz[2] = {iz * kPrimeZ, (iz + 1u) * kPrimeZ};
            // ix <= 2^11 never reaches bits 14..18 of the row, so the slice of a corner depends on (dy, dz) only: four tests,
            // and a hit brings both x-corners.
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t hyz = hy[q >> 1] ^ hz[q & 1];
                if (((hyz >> 14) & (uint32_t)(kSlices - 1)) != slice) continue;
#pragma unroll
                for (int dx = 0; dx < 2; ++dx) {
                    const int k = 4 * dx + q;   // corner (dx, dy, dz) = (dx, q>>1, q&1)
                    float *dst = acc + 2u * (((ix + dx) ^ hyz) & (uint32_t)(kSliceRows - 1));
                    atomicAdd(dst, corner_weight(c, k, g0));
                    atomicAdd(dst + 1, corner_weight(c, k, g1));
                }
            }
        }
    }
    SC_STAMP(2);
    __syncthreads();
    SC_STAMP(3);
    float *out = G + 2 * (size_t)slice * kSliceRows;
    if (replicas == 1) {
        for (uint32_t i = threadIdx.x; i < 2u * kSliceRows; i += blockDim.x) out[i] = acc[i];
    } else {
        for (uint32_t i = threadIdx.x; i < 2u * kSliceRows; i += blockDim.x) {
            const float v = acc[i];
            if (v != 0.0f) atomicAdd(out + i, v);
        }
    }
    SC_STAMP(4);
}

#ifdef NSIG_DEC_TIMING
NSIG_EXPORT int scatter_timing_stamps(unsigned long long *out8) {
    return hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_scatter_stamps), sizeof(unsigned long long) * 8) == hipSuccess ? 0 : 1;
}
#endif

// Owner-computes scatter of one base level's feature gradient (stage-1 training): as k_scatter_sliced, with the level's
// own resolution (not a power of two, so the cell index uses the same IEEE divisions as the forward: corner_rows()).
__global__ void __launch_bounds__(1024) k_scatter_level(const float *__restrict__ xyzs, float bound, const float2 *__restrict__ dplane, uint32_t M,
                                                        float cell, float *__restrict__ G) {
    extern __shared__ float acc[];
    const uint32_t slice = blockIdx.x >> 3, replica = blockIdx.x & 7u;
    for (uint32_t i = threadIdx.x; i < 2u * kSliceRows; i += blockDim.x) acc[i] = 0.0f;
    __syncthreads();
    const uint32_t chunk = ceil_div(M, (uint32_t)kReplicas);
    const uint32_t beg = min(M, replica * chunk), end = min(M, beg + chunk);
    const float two_b = 2.0f * bound;
    for (uint32_t m = beg + threadIdx.x; m < end; m += blockDim.x) {
        const float2 g = dplane[m];
        if (g.x == 0.0f && g.y == 0.0f) continue;
        Corner8 c;
        corner_rows((xyzs[3 * (size_t)m] + bound) / two_b, (xyzs[3 * (size_t)m + 1] + bound) / two_b, (xyzs[3 * (size_t)m + 2] + bound) / two_b, cell, c);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if ((c.row[k] >> 14) != slice) continue;
            float *dst = acc + 2u * (c.row[k] & (kSliceRows - 1));
            atomicAdd(dst, corner_weight(c, k, g.x));
            atomicAdd(dst + 1, corner_weight(c, k, g.y));
        }
    }
    __syncthreads();
    float *out = G + 2 * (size_t)slice * kSliceRows;
    for (uint32_t i = threadIdx.x; i < 2u * kSliceRows; i += blockDim.x) {
        const float v = acc[i];
        if (v != 0.0f) atomicAdd(out + i, v);
    }
}

// ----------------------------------------------------------------------------- binned scatter
//
// Two measurements shape this version (tools/micro/lds_atomic_rate.hip, tools/scatter_timing.py):
//  * ds_add_f32 retires 0.33 lane-operations per clock per CU; ds_add_u64 4.4 (ds_add_u32 5.2).  The scatter's 20.6 M LDS float
//    atomics alone are 100 us -- that, not the instruction count, bounded k_scatter_sliced.  So the owners accumulate in 64-bit
//    FIXED POINT: contribution * 2^k rounded to an integer, k chosen from the largest |gradient| of the launch and the slice's
//    entry count so that no row sum can overflow (fixed_scale); the integer sum is exact and independent of the order of the
//    atomics, and the owner converts back once per row.
//  * with 16 bytes per (row, feature pair) an LDS slice holds 8192 rows: 64 slices.  Letting every owner test every point would
//    double the redundant work, so the (point, (dy,dz) pair) hits are first grouped by slice with an exact two-pass counting
//    sort -- count, then write at atomically reserved positions -- and an owner streams only its own entries.  An entry is
//    self-contained (16 bytes: x cell, the pair's 13 row bits, the x weight, the two gradients already multiplied by the y and
//    z weights); gathering 32-byte records at random from the 41 MB array instead made this slower than what it replaced.
// The slice of a pair depends on (iy, iz, dy, dz) only (ix < 2^12 stays below bit 13), and a hit carries both x corners.
static_assert(kBinRows == 8192, "slice layout");   // constants and BinHeader: hashgrid.h

__device__ inline bool record_pairs(const uint4 *__restrict__ rec4, uint32_t m, uint32_t (&slices)[4], float &gabs) {
    const uint4 ra = rec4[2 * (size_t)m], rb = rec4[2 * (size_t)m + 1];
    const float g0 = __uint_as_float(rb.y), g1 = __uint_as_float(rb.z);
    if (g0 == 0.0f && g1 == 0.0f) return false;   // padding rows and terminated rays
    gabs = __uint_as_float(max(__float_as_uint(g0) & 0x7fffffffu, __float_as_uint(g1) & 0x7fffffffu));   // integer max of |bits|: a NaN stays visible
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) slices[q] = pair_slice(pair_hash(ra.x >> 16, ra.y, q));
    return true;
}

// Pass 1: wg[w][s] = entries of slice s among the chunks of workgroup w (plain stores: no global atomics); gmax = max |gradient|.
// (all four kernels: blockIdx.y = record set -- one for the codebook, 16 base levels in stage-1 training)
__global__ void __launch_bounds__(kBinThreads) k_bin_count(const float *__restrict__ rec_all, uint32_t M, BinHeader *__restrict__ hd_all) {
    const float *__restrict__ rec = rec_all + (size_t)blockIdx.y * M * 8;
    BinHeader *__restrict__ hd = hd_all + blockIdx.y;
    __shared__ uint32_t h[kBinSlices], gm;
    if (threadIdx.x < kBinSlices) h[threadIdx.x] = 0;
    if (threadIdx.x == 0) gm = 0;
    __syncthreads();
    uint32_t gb = 0;
    for (uint32_t m = blockIdx.x * kBinThreads + threadIdx.x; m < M; m += gridDim.x * kBinThreads) {
        uint32_t sl[4];
        float gabs;
        if (record_pairs(reinterpret_cast<const uint4 *>(rec), m, sl, gabs)) {
#pragma unroll
            for (int q = 0; q < 4; ++q) atomicAdd(&h[sl[q]], 1u);
            gb = max(gb, __float_as_uint(gabs));   // non-negative floats (and +inf, NaN) order like their bit patterns
        }
    }
    gb = wave_max(gb);
    if ((threadIdx.x & 63) == 0 && gb) atomicMax(&gm, gb);
    __syncthreads();
    if (threadIdx.x < kBinSlices) hd->wg[blockIdx.x][threadIdx.x] = h[threadIdx.x];
    if (threadIdx.x == 0 && gm) atomicMax(&hd->gmax_bits, gm);
}

// One workgroup: slice totals, slice starts, and every (workgroup, slice) write offset -- the queue order is a pure function of
// the input, so the whole scatter is reproducible bit for bit up to the final float adds of the four replicas.
__global__ void __launch_bounds__(1024) k_bin_scan(BinHeader *__restrict__ hd_all, uint32_t n_wg) {
    BinHeader *__restrict__ hd = hd_all + blockIdx.x;
    __shared__ uint32_t seg[16][kBinSlices], start[kBinSlices];
    const uint32_t s = threadIdx.x & (kBinSlices - 1), g = threadIdx.x >> 6;   // 16 segments of 16 workgroups
    uint32_t c[16], sum = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const uint32_t w = g * 16 + i;
        c[i] = w < n_wg ? hd->wg[w][s] : 0u;
        sum += c[i];
    }
    seg[g][s] = sum;
    __syncthreads();
    if (threadIdx.x < kBinSlices) {
        uint32_t tot = 0;
        for (int k = 0; k < 16; ++k) tot += seg[k][threadIdx.x];
        hd->counts[threadIdx.x] = tot;
        start[threadIdx.x] = tot;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t run = 0;
        for (uint32_t k = 0; k < kBinSlices; ++k) {
            const uint32_t t = start[k];
            start[k] = run;
            run += t;
        }
    }
    __syncthreads();
    uint32_t off = start[s];
    for (uint32_t k = 0; k < g; ++k) off += seg[k][s];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const uint32_t w = g * 16 + i;
        if (w < n_wg) hd->wg[w][s] = off;
        off += c[i];
    }
}

// Pass 2: queue[offset of (w, s) + rank] = entry
__global__ void __launch_bounds__(kBinThreads) k_bin_write(const float *__restrict__ rec_all, uint32_t M, const BinHeader *__restrict__ hd_all,
                                                           uint4 *__restrict__ queue_all) {
    const float *__restrict__ rec = rec_all + (size_t)blockIdx.y * M * 8;
    const BinHeader *__restrict__ hd = hd_all + blockIdx.y;
    uint4 *__restrict__ queue = queue_all + (size_t)blockIdx.y * 4 * M;
    __shared__ uint32_t h[kBinSlices], running[kBinSlices];
    if (threadIdx.x < kBinSlices) running[threadIdx.x] = hd->wg[blockIdx.x][threadIdx.x];
    const uint4 *__restrict__ rec4 = reinterpret_cast<const uint4 *>(rec);
    for (uint32_t m0 = blockIdx.x * kBinThreads; m0 < M; m0 += gridDim.x * kBinThreads) {   // uniform trip count: barriers inside
        if (threadIdx.x < kBinSlices) h[threadIdx.x] = 0;
        __syncthreads();
        const uint32_t m = m0 + threadIdx.x;
        uint32_t sl[4], local[4];
        float gabs;
        const bool live = m < M && record_pairs(rec4, m, sl, gabs);
        if (live)
#pragma unroll
            for (int q = 0; q < 4; ++q) local[q] = atomicAdd(&h[sl[q]], 1u);
        __syncthreads();
        if (live) {
            const uint4 ra = rec4[2 * (size_t)m], rb = rec4[2 * (size_t)m + 1];
            const float wy = __uint_as_float(ra.w), wz = __uint_as_float(rb.x);
            const float g0 = __uint_as_float(rb.y), g1 = __uint_as_float(rb.z);
#pragma unroll
            for (uint32_t q = 0; q < 4; ++q)
                queue[running[sl[q]] + local[q]] = pair_entry(ra.x & 0xffffu, pair_hash(ra.x >> 16, ra.y, q), __uint_as_float(ra.z), wy, wz, g0, g1, q);
        }
        __syncthreads();
        if (threadIdx.x < kBinSlices) running[threadIdx.x] += h[threadIdx.x];
    }
}

// ---- planned variant: where an entry goes depends on the point's position only, so the count, the scan and the destinations
// are computed from xyzs while the forward pass is still running (off the critical path, on a side stream), and k_field_bwd
// writes its gradients straight into the queue: no 32-byte record round trip and no binning passes between the MLP backward
// and the owners.  Every point gets its four entries (a zero gradient adds zero).
__device__ inline void point_slices(const float *__restrict__ xyzs, uint32_t m, float bound, uint32_t (&sl)[4]) {
    const float two_b = 2.0f * bound;
    uint32_t iy, iz;
    float w;
    codebook_axis((xyzs[3 * (size_t)m + 1] + bound) / two_b, iy, w);
    codebook_axis((xyzs[3 * (size_t)m + 2] + bound) / two_b, iz, w);
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) sl[q] = pair_slice(pair_hash(iy, iz, q));
}

// rows_dev (hg_scatter_plan_rows; both kernels): the point count lives on the device, M is the capacity the launch and the plan were sized for -- rows beyond
// *rows_dev get no entries, workgroups beyond them count nothing (with *rows_dev == 0 the plan is the reset header: no entries, gmax_bits 0).
__global__ void __launch_bounds__(kBinThreads) k_plan_count(const float *__restrict__ xyzs, uint32_t M, float bound, BinHeader *__restrict__ hd,
                                                            const uint32_t *__restrict__ rows_dev = nullptr) {
    __shared__ uint32_t h[kBinSlices];
    if (rows_dev != nullptr) M = min(M, *rows_dev);
    if (threadIdx.x < kBinSlices) h[threadIdx.x] = 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) hd->gmax_bits = 0;   // k_field_bwd raises it (stream-ordered after the plan)
    __syncthreads();
    for (uint32_t m = blockIdx.x * kBinThreads + threadIdx.x; m < M; m += gridDim.x * kBinThreads) {
        uint32_t sl[4];
        point_slices(xyzs, m, bound, sl);
#pragma unroll
        for (int q = 0; q < 4; ++q) atomicAdd(&h[sl[q]], 1u);
    }
    __syncthreads();
    if (threadIdx.x < kBinSlices) hd->wg[blockIdx.x][threadIdx.x] = h[threadIdx.x];
}

// Every workgroup derives its own write offsets from the count table (wg[w][s], 64 KiB at most, L2-resident): slice starts = exclusive
// prefix over the slice totals, plus what the workgroups in front of it found for that slice -- the single-workgroup scan launch that
// used to sit between the two passes (k_bin_scan: 2-16 us in a chain of small launches) is gone.  Workgroup 0 stores the slice totals
// the owners read.  Same queue order as count -> scan -> dest.
__global__ void __launch_bounds__(kBinThreads) k_plan_dest(const float *__restrict__ xyzs, uint32_t M, float bound, BinHeader *__restrict__ hd,
                                                           uint4 *__restrict__ dest, const uint32_t *__restrict__ rows_dev = nullptr) {
    __shared__ uint32_t h[kBinSlices], running[kBinSlices], seg_tot[16][kBinSlices], seg_before[16][kBinSlices];
    if (rows_dev != nullptr) M = min(M, *rows_dev);      // (one value for the launch: the trip count below stays uniform per workgroup)
    {
        static_assert(kBinThreads == 16 * kBinSlices && kBinGrid == 256, "16 segments of 16 workgroups, one thread per (segment, slice)");
        const uint32_t s = threadIdx.x & (kBinSlices - 1), g = threadIdx.x >> 6, n_wg = gridDim.x;
        uint32_t tot = 0, before = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const uint32_t w = g * 16 + i;
            const uint32_t c = w < n_wg ? hd->wg[w][s] : 0u;
            tot += c;
            if (w < blockIdx.x) before += c;
        }
        seg_tot[g][s] = tot;
        seg_before[g][s] = before;
        __syncthreads();
        if (threadIdx.x < kBinSlices) {      // one wave: slice totals, their exclusive prefix, this workgroup's offset inside each slice
            uint32_t t = 0, b = 0;
#pragma unroll
            for (int k = 0; k < 16; ++k) { t += seg_tot[k][threadIdx.x]; b += seg_before[k][threadIdx.x]; }
            const uint32_t incl = wave_prefix_sum(t, (int)threadIdx.x);
            running[threadIdx.x] = incl - t + b;
            if (blockIdx.x == 0) hd->counts[threadIdx.x] = t;
        }
    }
    for (uint32_t m0 = blockIdx.x * kBinThreads; m0 < M; m0 += gridDim.x * kBinThreads) {   // uniform trip count: barriers inside
        if (threadIdx.x < kBinSlices) h[threadIdx.x] = 0;
        __syncthreads();
        const uint32_t m = m0 + threadIdx.x;
        uint32_t sl[4], local[4];
        if (m < M) {
            point_slices(xyzs, m, bound, sl);
#pragma unroll
            for (int q = 0; q < 4; ++q) local[q] = atomicAdd(&h[sl[q]], 1u);
        }
        __syncthreads();
        if (m < M) dest[m] = make_uint4(running[sl[0]] + local[0], running[sl[1]] + local[1], running[sl[2]] + local[2], running[sl[3]] + local[3]);
        __syncthreads();
        if (threadIdx.x < kBinSlices) running[threadIdx.x] += h[threadIdx.x];
    }
}

// ---- the planned variant over the 16 base levels (stage-1 training: every base table has its own gradient).  blockIdx.y = level,
// blockIdx.x = a CHUNK of 1024 consecutive sample points (consecutive samples of a few rays).
// Where an entry goes depends on the sample positions and the level's cell only, so the counting and the offsets are computed beside the
// forward pass (hg_levels_plan: k_levels_count -> k_levels_scan); behind the MLP backward one pass turns the feature gradients into queue
// entries (k_level_entries) and the 16 x 64 slice owners run (k_scatter_binned).  Three things differ from the codebook's planned scatter:
//   * the point count is a device value (`rows_dev`, may be null): a captured step sizes its launches for the buffers' capacity M and walks
//     only the rows the march produced;
//   * a chunk's entries are sorted by slice in LDS and leave as whole 128-byte lines (a run of a slice's entries is contiguous in the queue):
//     written straight from the lanes -- 64 lanes, 64 different lines per store -- the pass was bound by the L2's request rate (82 us for
//     8 M entries); the per-point destination array of the first version (32 MB written by the plan, read here) is gone: a chunk needs its
//     64 run offsets only;
//   * MERGED RUNS on the coarse levels.  A ray's consecutive samples share a cell there (level 0: ~37 samples per cell), i.e. the same 8 rows;
//     worse, a coarse level has few distinct (y, z) cell pairs, so the slices -- bits of hash(y, z) -- are loaded very unevenly and ONE owner
//     streamed 10-20 % of a level's entries (87 us at level 0 against 12.5 us at the fine levels, profiles/r05_stage1_steps.txt).  For levels
//     < kMergeLevels the wave adds up each run of lanes in the same cell first (16 corner-feature sums, fp32, fixed lane order) and only the
//     run's first lane emits entries: two per (dy, dz) pair, one for each x side (x weight 0 and 1: the owner's (1 - wx, wx) split then routes
//     the sum to one row).  Level 0 shrinks 18-fold.  The sums differ from the unmerged ones by fp32 rounding of the partial sums (1e-7).
constexpr uint32_t kMergeLevels = 10;        // resolutions 16..294: >= 2 samples per cell along a ray at the bench step length
constexpr uint32_t kLevelQueueStride = 8;    // queue entries reserved per point and level (a merged level whose every point is its own run emits 8)
constexpr uint32_t kLevelStage = 4 * kBinThreads;   // entries a chunk sorts in LDS (64 KiB: two workgroups per compute unit, or one beside the weight-gradient kernel);
                                                    // a merged chunk with more (runs shorter than two samples on average) stores its entries straight from the lanes

struct LevelsPlan {
    BinHeader *hd;          // [16]
    uint32_t *chunk_tab;    // [16][n_chunks][64]: entries of slice s in chunk c, then (k_levels_scan) the queue offset of that run
    uint32_t *chunk_max;    // [16][n_chunks]: max |contribution| among a chunk's entries, as a float bit pattern (0 for chunks past the live rows)
    uint4 *queue;           // [16][8 M]
    uint32_t n_chunks;
};
static size_t levels_plan_bytes(uint32_t M) {
    const size_t n_chunks = ceil_div(M, kBinThreads);
    return (size_t)NSIG_BASE_LEVELS * (sizeof(BinHeader) + n_chunks * (kBinSlices + 4) * sizeof(uint32_t) + (size_t)kLevelQueueStride * M * sizeof(uint4));
}
static LevelsPlan levels_plan_view(void *plan, uint32_t M) {
    LevelsPlan v;
    v.n_chunks = ceil_div(M, kBinThreads);
    v.hd = reinterpret_cast<BinHeader *>(plan);
    v.chunk_tab = reinterpret_cast<uint32_t *>(v.hd + NSIG_BASE_LEVELS);
    v.chunk_max = v.chunk_tab + (size_t)NSIG_BASE_LEVELS * v.n_chunks * kBinSlices;
    v.queue = reinterpret_cast<uint4 *>(v.chunk_max + (size_t)NSIG_BASE_LEVELS * v.n_chunks * 4);     // (16-byte aligned: 64 + 4 words per chunk and level; a quarter of the second block is used)
    return v;
}

struct LevelPoint {
    uint32_t ix, iy, iz;
    float wx, wy, wz;
};
__device__ inline void level_point(const float *__restrict__ xyzs, uint32_t m, float bound, float cell, LevelPoint &p) {
    const float two_b = 2.0f * bound;
    axis_cell((xyzs[3 * (size_t)m] + bound) / two_b, cell, p.ix, p.wx);
    axis_cell((xyzs[3 * (size_t)m + 1] + bound) / two_b, cell, p.iy, p.wy);
    axis_cell((xyzs[3 * (size_t)m + 2] + bound) / two_b, cell, p.iz, p.wz);
}
// does this lane open a run?  (merged levels: first lane of a 16-lane row -- the runs are added up with DPP row shifts, which stay inside a
// row --, or another cell than the lane below; other levels: every live lane)
__device__ inline bool run_leader(bool merged, bool live, const LevelPoint &p) {
    if (!merged) return live;
    const uint32_t key = live ? (p.ix | (p.iy << 10) | (p.iz << 20)) : 0xffffffffu;      // resolutions < 1024 on the merged levels
    const uint32_t below = (uint32_t)__builtin_amdgcn_update_dpp((int)~key, (int)key, 0x111, 0xf, 0xf, false);      // row_shr:1 (lane 0 of a row keeps ~key)
    return live && key != below;
}

__global__ void __launch_bounds__(kBinThreads) k_levels_count(const float *__restrict__ xyzs, uint32_t M, const uint32_t *__restrict__ rows_dev, float bound,
                                                              LevelGeom geom, LevelsPlan pl) {
    const uint32_t level = blockIdx.y, chunk = blockIdx.x;
    const uint32_t n = rows_dev != nullptr ? min(M, *rows_dev) : M;
    if (chunk * kBinThreads >= n) return;
    __shared__ uint32_t h[kBinSlices];
    if (threadIdx.x < kBinSlices) h[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t m = chunk * kBinThreads + threadIdx.x;
    const bool live = m < n, merged = level < kMergeLevels;
    LevelPoint p{};
    if (live) level_point(xyzs, m, bound, geom.cell[level], p);
    if (run_leader(merged, live, p)) {
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) atomicAdd(&h[pair_slice(pair_hash(p.iy, p.iz, q))], merged ? 2u : 1u);
    }
    __syncthreads();
    if (threadIdx.x < kBinSlices) pl.chunk_tab[((size_t)level * pl.n_chunks + chunk) * kBinSlices + threadIdx.x] = h[threadIdx.x];
}

// One workgroup per level: slice totals (what the owners read), slice starts, and -- in place of the counts -- the queue offset of every
// (chunk, slice) run: the queue is slice-major, a slice's runs in chunk order.  16 segments of chunks x 64 slices = 1024 threads.
__global__ void __launch_bounds__(kBinThreads) k_levels_scan(uint32_t M, const uint32_t *__restrict__ rows_dev, LevelsPlan pl) {
    const uint32_t level = blockIdx.x;
    const uint32_t n = rows_dev != nullptr ? min(M, *rows_dev) : M;
    const uint32_t chunks = ceil_div(n, kBinThreads), per = ceil_div(chunks, 16u);
    uint32_t *__restrict__ tab = pl.chunk_tab + (size_t)level * pl.n_chunks * kBinSlices;
    __shared__ uint32_t seg[16][kBinSlices], start[kBinSlices];
    const uint32_t s = threadIdx.x & (kBinSlices - 1), g = threadIdx.x >> 6;
    const uint32_t c0 = min(chunks, g * per), c1 = min(chunks, c0 + per);
    uint32_t sum = 0;
    for (uint32_t c = c0; c < c1; ++c) sum += tab[(size_t)c * kBinSlices + s];
    seg[g][s] = sum;
    __syncthreads();
    if (threadIdx.x < kBinSlices) {      // one wave: totals and their exclusive prefix
        uint32_t t = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) t += seg[k][threadIdx.x];
        const uint32_t incl = wave_prefix_sum(t, (int)threadIdx.x);
        start[threadIdx.x] = incl - t;
        pl.hd[level].counts[threadIdx.x] = t;
    }
    __syncthreads();
    uint32_t off = start[s];
    for (uint32_t k = 0; k < g; ++k) off += seg[k][s];
    for (uint32_t c = c0; c < c1; ++c) {
        const uint32_t t = tab[(size_t)c * kBinSlices + s];
        tab[(size_t)c * kBinSlices + s] = off;
        off += t;
    }
}

// sum over the run of lanes [lane, run_end] of this 16-lane row, delivered to `lane` (meaningful at a run's first lane): four row shifts, no LDS
template <int D>
__device__ inline float row_shl(float v) {      // lane i reads lane i + D of its row (0 past the row's end)
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x100 + D, 0xf, 0xf, true));
}
// the maximum over the wave's 64 lanes (all active), the same value in every lane: four row shifts, then the four rows' first lanes
__device__ inline uint32_t wave_max_u32(uint32_t v) {
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x101, 0xf, 0xf, true));
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x102, 0xf, 0xf, true));
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x104, 0xf, 0xf, true));
    v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x108, 0xf, 0xf, true));
    return max(max((uint32_t)__builtin_amdgcn_readlane((int)v, 0), (uint32_t)__builtin_amdgcn_readlane((int)v, 16)),
               max((uint32_t)__builtin_amdgcn_readlane((int)v, 32), (uint32_t)__builtin_amdgcn_readlane((int)v, 48)));
}
__device__ inline float run_sum(float v, uint32_t l16, uint32_t run_end) {
    float o = row_shl<1>(v);
    v += l16 + 1u <= run_end ? o : 0.0f;
    o = row_shl<2>(v);
    v += l16 + 2u <= run_end ? o : 0.0f;
    o = row_shl<4>(v);
    v += l16 + 4u <= run_end ? o : 0.0f;
    o = row_shl<8>(v);
    v += l16 + 8u <= run_end ? o : 0.0f;
    return v;
}

#ifdef NSIG_ENT_TIMING      // diagnostic build: where a workgroup of k_level_entries spends its time (10 ns ticks, summed over workgroups, per level; [level][8] = workgroups counted)
__device__ unsigned long long g_ent_phase[16][9];
#define ENT_STAMP(k)                                                                                          \
    do {                                                                                                      \
        if (threadIdx.x == 0) {                                                                               \
            const unsigned long long now_ = wall_clock64();                                                   \
            atomicAdd(&g_ent_phase[level][k], now_ - ent_t_);                                                  \
            if ((k) == 7) atomicAdd(&g_ent_phase[level][8], 1ull);                                             \
            ent_t_ = now_;                                                                                    \
        }                                                                                                     \
    } while (0)
#else
#define ENT_STAMP(k)
#endif

// feature gradients of a chunk's points at one level -> queue entries, sorted by slice in LDS, stored as contiguous runs; raises the level's
// max |contribution| (the owners' fixed-point scale)
__global__ void __launch_bounds__(kBinThreads) k_level_entries(const float *__restrict__ xyzs, uint32_t M, const uint32_t *__restrict__ rows_dev, float bound,
                                                               const float2 *__restrict__ dplanes, uint32_t stride, LevelGeom geom, LevelsPlan pl) {
    extern __shared__ __attribute__((aligned(16))) uint4 staged[];      // [kLevelStage]
    __shared__ uint32_t h[kBinSlices], base[kBinSlices + 1], roff[kBinSlices], wg_max;
    __shared__ uint8_t slice_of[kLevelStage];      // which slice's run a staged entry belongs to
    const uint32_t level = blockIdx.y, chunk = blockIdx.x;
#ifdef NSIG_ENT_TIMING
    unsigned long long ent_t_ = wall_clock64();
#endif
    // every input requested before the row count is known (rows past it are inside the buffers, their values unused): one memory latency at the
    // head of the workgroup instead of three in a chain (count -> positions -> gradients); two 1024-thread workgroups per unit hide little
    const uint32_t m = chunk * kBinThreads + threadIdx.x, lane = threadIdx.x & 63u, mc = min(m, M - 1u);
    const float px = xyzs[3 * (size_t)mc], py = xyzs[3 * (size_t)mc + 1], pz = xyzs[3 * (size_t)mc + 2];
    float2 g = dplanes[(size_t)level * stride + mc];
    const uint32_t my_roff = threadIdx.x < kBinSlices ? pl.chunk_tab[((size_t)level * pl.n_chunks + chunk) * kBinSlices + threadIdx.x] : 0u;
    const uint32_t n = rows_dev != nullptr ? min(M, *rows_dev) : M;
    if (chunk * kBinThreads >= n) {
        if (threadIdx.x == 0) pl.chunk_max[(size_t)level * pl.n_chunks + chunk] = 0u;
        return;
    }
    if (threadIdx.x < kBinSlices) {
        h[threadIdx.x] = 0;
        roff[threadIdx.x] = my_roff;      // where this chunk's run of each slice starts in the queue
    }
    if (threadIdx.x == 0) wg_max = 0;
    __syncthreads();
    ENT_STAMP(0);      // inputs arrived (the row count, the run offsets)
    const bool live = m < n, merged = level < kMergeLevels;
    LevelPoint p{};
    if (live) {
        const float two_b = 2.0f * bound, cell = geom.cell[level];
        axis_cell((px + bound) / two_b, cell, p.ix, p.wx);
        axis_cell((py + bound) / two_b, cell, p.iy, p.wy);
        axis_cell((pz + bound) / two_b, cell, p.iz, p.wz);
    } else {
        g = make_float2(0.0f, 0.0f);
    }
    const bool leader = run_leader(merged, live, p);
    uint32_t sl[4], hyz[4], rank[4];
    if (leader) {
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) {
            hyz[q] = pair_hash(p.iy, p.iz, q);
            sl[q] = pair_slice(hyz[q]);
            rank[q] = atomicAdd(&h[sl[q]], merged ? 2u : 1u);
        }
    }
    ENT_STAMP(1);      // cells, leaders, ranks
    // merged levels: the 16 corner-feature contributions of a run, summed into its first lane
    float c[4][2][2];      // [(dy, dz) pair][x side][feature]
    uint32_t gb = max(__float_as_uint(g.x) & 0x7fffffffu, __float_as_uint(g.y) & 0x7fffffffu);
    if (merged) {
        const uint32_t l16 = lane & 15u;
        const uint32_t row_leaders = (uint32_t)(__ballot(leader || !live) >> (lane & 48u)) & 0xffffu;
        const uint32_t higher = row_leaders & ~((2u << l16) - 1u);
        const uint32_t run_end = higher ? (uint32_t)__ffs((int)higher) - 2u : 15u;
        gb = 0;
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) {
            const float fz = (q & 1u) ? p.wz : 1.0f - p.wz, fy = (q >> 1) ? p.wy : 1.0f - p.wy;
            const float a0 = (g.x * fz) * fy, a1 = (g.y * fz) * fy;      // corner_weight()'s order; zero on dead lanes
            c[q][0][0] = run_sum(a0 * (1.0f - p.wx), l16, run_end);
            c[q][0][1] = run_sum(a1 * (1.0f - p.wx), l16, run_end);
            c[q][1][0] = run_sum(a0 * p.wx, l16, run_end);
            c[q][1][1] = run_sum(a1 * p.wx, l16, run_end);
            if (leader)
#pragma unroll
                for (int t = 0; t < 4; ++t) gb = max(gb, __float_as_uint(c[q][t >> 1][t & 1]) & 0x7fffffffu);
        }
    }
    ENT_STAMP(2);      // run sums
    __syncthreads();
    ENT_STAMP(3);      // barrier
    if (threadIdx.x < kBinSlices) {      // one wave: where each slice's run starts in the staging area
        const uint32_t t = h[threadIdx.x];
        const uint32_t incl = wave_prefix_sum(t, (int)threadIdx.x);
        base[threadIdx.x] = incl - t;
        if (threadIdx.x == kBinSlices - 1) base[kBinSlices] = incl;
    }
    __syncthreads();
    ENT_STAMP(4);      // prefix + barrier
    const uint32_t total = base[kBinSlices];
    const bool direct = total > kLevelStage;      // (uniform; merged levels only)
    uint4 *__restrict__ queue = pl.queue + (size_t)level * kLevelQueueStride * M;
    if (leader) {
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) {
            uint4 e0, e1 = make_uint4(0u, 0u, 0u, 0u);
            if (merged) {
                const uint32_t key = p.ix | ((hyz[q] & (kBinRows - 1)) << 16);
                e0 = make_uint4(key, __float_as_uint(0.0f), __float_as_uint(c[q][0][0]), __float_as_uint(c[q][0][1]));
                e1 = make_uint4(key, __float_as_uint(1.0f), __float_as_uint(c[q][1][0]), __float_as_uint(c[q][1][1]));
            } else {
                e0 = pair_entry(p.ix, hyz[q], p.wx, p.wy, p.wz, g.x, g.y, q);
            }
            // (two spelled-out branches: one pointer that may address LDS or global memory becomes a FLAT store -- 50 us of this kernel's 66)
            if (direct) {
                uint4 *__restrict__ dst = queue + roff[sl[q]] + rank[q];
                dst[0] = e0;
                if (merged) dst[1] = e1;
            } else {
                const uint32_t at = base[sl[q]] + rank[q];
                staged[at] = e0;
                slice_of[at] = (uint8_t)sl[q];
                if (merged) {
                    staged[at + 1] = e1;
                    slice_of[at + 1] = (uint8_t)sl[q];
                }
            }
        }
    }
    ENT_STAMP(5);      // staging writes
    __syncthreads();
    ENT_STAMP(6);      // barrier
    // Copy-out: consecutive lanes take consecutive entries of a run = whole lines.  At most kLevelStage / kBinThreads = 4 entries per thread; all of a thread's LDS reads of
    // one kind are issued together (as a loop over j this was, per entry, two dependent LDS round trips in front of its store: the workgroup's last phase, 25-42 % of its
    // time -- and a workgroup's time is what this launch is made of: two workgroups per unit, ~9 us each, 19 rounds of them at 620 k points).  The empty asm statements
    // pin the reads in front of the tests that guard the stores (a read used only behind a test is sunk behind it).
    if (!direct && total != 0u) {      // (uniform)
        typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
        constexpr uint32_t kPer = kLevelStage / kBinThreads;
        uint32_t sj[kPer], ro[kPer], ba[kPer];
        u32x4_t e[kPer];
#pragma unroll
        for (uint32_t u = 0; u < kPer; ++u) {
            const uint32_t j = min(threadIdx.x + u * kBinThreads, total - 1u);
            sj[u] = slice_of[j];
            const uint4 t = staged[j];
            e[u] = u32x4_t{t.x, t.y, t.z, t.w};
        }
#pragma unroll
        for (uint32_t u = 0; u < kPer; ++u) asm volatile("" : "+v"(sj[u]));
#pragma unroll
        for (uint32_t u = 0; u < kPer; ++u) {
            ro[u] = roff[sj[u]];
            ba[u] = base[sj[u]];
        }
#pragma unroll
        for (uint32_t u = 0; u < kPer; ++u) asm volatile("" : "+v"(ro[u]), "+v"(ba[u]), "+v"(e[u]));
#pragma unroll
        for (uint32_t u = 0; u < kPer; ++u) {
            const uint32_t j = threadIdx.x + u * kBinThreads;
            // streamed out: a queue line is written here once and read once by an owner on some other XCD -- no L2 can serve it (the launch itself takes the same time; the
            // step is 1 % shorter for what the caches keep instead: same box, two rounds, 1.201 / 1.198 -> 1.189 / 1.187 ms with the owners' loads streamed as well)
            if (j < total) __builtin_nontemporal_store(e[u], reinterpret_cast<u32x4_t *>(queue + ro[u] + (j - ba[u])));
        }
    }
    // the chunk's max |contribution|: a plain store; the level's owners take the maximum over the chunks themselves.  (One word per level raised with
    // atomics by 31 k waves -- the codebook scatter's scheme, where 3 k waves do it -- was the largest single item of this kernel.)  The wave's maximum by
    // lane exchanges (left to the compiler, `if (gb) atomicMax(...)` becomes a scalar loop over the wave's lanes), one LDS operation per wave.
    gb = wave_max_u32(gb);
    if (lane == 0 && gb) atomicMax(&wg_max, gb);      // (LDS)
    __syncthreads();
    if (threadIdx.x == 0) pl.chunk_max[(size_t)level * pl.n_chunks + chunk] = wg_max;
    ENT_STAMP(7);      // copy-out issued, maximum raised
}

#ifdef NSIG_ENT_TIMING
NSIG_EXPORT int level_entries_phase_ticks(unsigned long long *out144, int reset) {
    if (hipMemcpyFromSymbol(out144, HIP_SYMBOL(g_ent_phase), sizeof(unsigned long long) * 144) != hipSuccess) return 1;
    if (reset) {
        unsigned long long zero[144] = {};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_ent_phase), zero, sizeof(zero)) != hipSuccess) return 1;
    }
    return 0;
}
#endif

// (a single-precision formulation of this conversion -- t = c * 2^(k-27) split into its integer part and a 27-bit fraction, two exact cvt_i32 -- changes nothing,
// also with the owners' loads really in flight: 369-375 us against 365-373 on the 16-level scatter; the f64 instructions are ~5 us of the owners, LABNOTES 17a)
__device__ inline long long to_fixed(float c, int k) { return __double2ll_rn(ldexp((double)c, k)); }

// The fixed-point scale k of a slice (contribution c -> round(c * 2^k)), shared by the owners and the merge so that the two cannot disagree.
// Every |contribution| <= gmax < 2^E and a row receives at most one per entry of its slice, so a row's |sum| <= n * gmax < 2^(E + bits(n)):
// k = 62 - E - bits(n) keeps it below 2^62 (rounding adds at most n / 2).  Up to 2^11 entries the scale stays at 51 - E, 2^-51 of the
// maximum.  This holds for ANY distribution of the entries over the rows: one row may take all of them (every sample of a launch on one
// vertex) -- the codebook's routes once assumed 2^11 hits per row at most and wrapped modulo 2^64 beyond.  n is the slice's total entry
// count, not one replica's share: the merge adds the replicas' sums.  gmax_bits: a float bit pattern below +inf (a poisoned launch uses no scale).
__device__ inline int fixed_scale(uint32_t gmax_bits, uint32_t n) {
    int E;
    frexpf(__uint_as_float(gmax_bits), &E);
    return n > 2048u ? 62 - E - (32 - __builtin_clz(n)) : 51 - E;
}

// The owners of hg_levels_scatter_adam finish with the optimiser step of their rows: a slice's gradient never leaves the chip (no 64 MiB of G written and read back,
// no table pass on the step's serial tail).  The update is adam.h's; scratch: adam_prepare_launch's two scalars per table ([set] = lr / (1 - beta1^t), [kAdamGroup + set] = 1 / sqrt(1 - beta2^t)).
struct OwnerAdam {
    float *p[NSIG_BASE_LEVELS], *m[NSIG_BASE_LEVELS], *v[NSIG_BASE_LEVELS];
    const float *scratch;
    float beta1, beta2, eps, grad_scale;
    uint32_t on;
};

// blockIdx.x = slice * replicas + replica: the slice's entries, split evenly over the replicas.  replicas == 1: the owner is
// alone and stores its rows (no atomics, no zero-fill of the table, bit-reproducible).  replicas > 1 (`slabs`: hashgrid.h, "Replicas ... merge EXACTLY"):
// every replica leaves its fixed-point accumulators as a slab and k_scatter_merge, the next launch, sums a slice's slabs as integers, converts once and adds
// ONE float per element to G -- the slice's sum is that of a single owner bit for bit, in whatever order the replicas (or the entries) ran; G itself
// accumulates over the launches of a step (block render, content render: a + b is commutative, so their order is immaterial too).  This is the
// determinism of the reference's embedding_dense_backward (hash_encoding_wtmk_bit.py:99-116 -> a sort + segmented reduce).  (Until round 6 the replicas
// each converted their partial sum and merged with float atomics: G moved by half an ulp from run to run, and Adam(eps = 1e-15) amplified that.  A merge
// inside this launch -- slabs, a ticket per slice, the last arriver sums -- needs an agent-scope release / acquire around the ticket, i.e. a write-back and an
// invalidate of the XCD's whole L2 per workgroup: 29 -> 150 us, profiles/r06_exact_merge_ab.txt.  A launch boundary gives the same visibility for one
// launch gap.)
// The fixed-point scale leaves room for as many maximal contributions as the slice has entries (fixed_scale): at level 0 of stage 1 a million samples
// share 4913 rows, and a codebook launch may put all of its points on one vertex.
// add_to_g (replicas == 1; hg_scatter_planned on a small launch): the single owner ADDS its rows to G as the merge would have -- see the end of the kernel.
// set_max (optional): [sets][n_set_max] partial maxima of |contribution| (float bit patterns) whose maximum replaces the header's gmax_bits.
__global__ void __launch_bounds__(1024) k_scatter_binned(const BinHeader *__restrict__ hd_all, const uint4 *__restrict__ queue_all, uint32_t M,
                                                         ScatterTargets tg, uint32_t replicas,
                                                         const uint32_t *__restrict__ set_max = nullptr, uint32_t n_set_max = 0, OwnerAdam adam = OwnerAdam{},
                                                         unsigned long long *__restrict__ slabs = nullptr, bool add_to_g = false) {
    extern __shared__ unsigned long long acc64[];  // [kBinRows][2] fixed point
    const BinHeader *__restrict__ hd = hd_all + blockIdx.y;
    const uint4 *__restrict__ queue = queue_all + (size_t)blockIdx.y * 4 * M;
    float *__restrict__ G = tg.g[blockIdx.y];
    const uint32_t slice = blockIdx.x / replicas, replica = blockIdx.x - slice * replicas;
    // An owner is alone on its compute unit (128 KiB of accumulators), so every latency at its head is exposed, and with few entries the head IS the owner (41 us of
    // the launch at 33 k points).  Order: the slice counts as ONE load per wave (was: up to 63 scalar loads, each waited for), then the first round of queue entries
    // and the chunk maxima REQUESTED, then the accumulators cleared and the maximum reduced while those are on their way.
    static_assert(kBinSlices == 64, "one slice count per lane");
    const uint32_t lane = threadIdx.x & 63u, cnt = hd->counts[lane];
    const uint32_t before = wave_sum(lane < slice ? cnt : 0u);
    const uint32_t start = (uint32_t)__builtin_amdgcn_readfirstlane((int)before);
    const uint32_t n = (uint32_t)__builtin_amdgcn_readfirstlane(__shfl((int)cnt, (int)slice, 64)), chunk = ceil_div(n, replicas);
    const uint32_t beg = min(n, replica * chunk), end = min(n, beg + chunk);
    // The queue walk, software-pipelined: a round's four entries per thread are requested one round ahead, and nothing in the loop is conditional.  (The first
    // form -- four clamped loads, then `if (beyond the end) break;` in front of each entry's work -- compiled to load, s_waitcnt vmcnt(0), convert, four atomics,
    // next load: every load is used only behind its own test, so the compiler sank it there, and a thread had ONE entry in flight whatever the unroll depth; the
    // owners ran at the latency of ~40 dependent streaming loads.)  Requests beyond the end load the slice's last entry again; nothing is added for them.
    constexpr int kAhead = 4;      // (2 / 4 / 8 entries ahead per thread: 375 / 369 / 370 us on the 16-level scatter at 671 k points, same box)
    typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
    const u32x4_t *__restrict__ q = reinterpret_cast<const u32x4_t *>(queue + start);
    const uint32_t round = blockDim.x * kAhead;
    u32x4_t cur[kAhead] = {}, nxt[kAhead];
    if (beg < end) {      // (uniform)
#pragma unroll
        for (int u = 0; u < kAhead; ++u) cur[u] = __builtin_nontemporal_load(q + min(beg + u * blockDim.x + threadIdx.x, end - 1));
    }
    // The scale: fixed_scale (from gmax and the slice's entry count n).  A non-finite gradient anywhere in the launch
    // (an overflowing scaled loss under torch's GradScaler) poisons every row of G with NaN, so that the scaler's inf check sees it
    // exactly as it sees the inf/NaN float sums of the reference's dense gradients and skips the step.
    uint32_t gb = hd->gmax_bits, mx = 0;
    __shared__ uint32_t smax;
    if (set_max != nullptr) {
        for (uint32_t i = threadIdx.x; i < n_set_max; i += blockDim.x) mx = max(mx, set_max[(size_t)blockIdx.y * n_set_max + i]);
        if (threadIdx.x == 0) smax = 0;
    }
    if (beg < end || adam.on)      // (uniform)
        for (uint32_t i = threadIdx.x; i < 2u * kBinRows; i += blockDim.x) acc64[i] = 0ull;
    __syncthreads();
    if (set_max != nullptr) {
        mx = wave_max(mx);
        if (lane == 0 && mx) atomicMax(&smax, mx);
        __syncthreads();
        gb = smax;
    }
    const bool poisoned = gb >= 0x7f800000u;
    const int k = poisoned ? 0 : fixed_scale(gb, n);
    float *out = G + 2 * (size_t)slice * kBinRows;
    if (beg >= end && !adam.on) {      // (uniform) nothing for this owner (two of level 0's 64 slices hold no cell pair at all; a replica beyond a short slice's end -- it leaves no slab, and the merge knows): its rows are zeros, no accumulators needed
        if (poisoned || (replicas == 1 && !add_to_g)) {
            const float f = poisoned ? __uint_as_float(0x7fc00000u) : 0.0f;
            for (uint32_t i4 = threadIdx.x; i4 < kBinRows / 2u; i4 += blockDim.x) *reinterpret_cast<float4 *>(out + 4u * i4) = make_float4(f, f, f, f);
        }
        return;
    }
    if (beg < end) {      // (uniform; an owner with the optimiser step inside comes here without entries too)
        for (uint32_t base = beg; base < end; base += round) {      // (uniform trip count)
#pragma unroll
            for (int u = 0; u < kAhead; ++u) nxt[u] = __builtin_nontemporal_load(q + min(base + round + u * blockDim.x + threadIdx.x, end - 1));
            __builtin_amdgcn_sched_barrier(0);      // (the requests stay in front of the round's work)
#pragma unroll
            for (int u = 0; u < kAhead; ++u) {
                if (base + u * blockDim.x + threadIdx.x < end) {      // (the requests are behind us: this test guards arithmetic and atomics only)
                    const uint32_t ix = cur[u][0] & 0xffffu, hyz = cur[u][0] >> 16;     // hyz: the pair's 13 row bits
                    const float wx = __uint_as_float(cur[u][1]), a0 = __uint_as_float(cur[u][2]), a1 = __uint_as_float(cur[u][3]);
                    unsigned long long *d0 = acc64 + 2u * ((ix ^ hyz) & (kBinRows - 1)), *d1 = acc64 + 2u * (((ix + 1u) ^ hyz) & (kBinRows - 1));
                    // (an entry of a merged level carries ONE x side -- wx is exactly 0 or 1 -- and the other side's two adds would add zeros)
                    if (wx != 1.0f) {
                        atomicAdd(d0, (unsigned long long)to_fixed(a0 * (1.0f - wx), k));
                        atomicAdd(d0 + 1, (unsigned long long)to_fixed(a1 * (1.0f - wx), k));
                    }
                    if (wx != 0.0f) {
                        atomicAdd(d1, (unsigned long long)to_fixed(a0 * wx, k));
                        atomicAdd(d1 + 1, (unsigned long long)to_fixed(a1 * wx, k));
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < kAhead; ++u) cur[u] = nxt[u];
        }
    }
    __syncthreads();
    if (adam.on) {      // (uniform; replicas == 1) the optimiser step of this slice's rows: parameters and moments in, the gradient from LDS, parameters and moments out
        constexpr uint32_t kTrips = kBinRows / 2u / 1024u;      // float4 (two rows) per thread: the launch has 1024 threads
        typedef float f32x4_t __attribute__((ext_vector_type(4)));
        const size_t first = (size_t)slice * (kBinRows / 2u);
        f32x4_t *pp = reinterpret_cast<f32x4_t *>(adam.p[blockIdx.y]) + first, *pm = reinterpret_cast<f32x4_t *>(adam.m[blockIdx.y]) + first,
                *pv = reinterpret_cast<f32x4_t *>(adam.v[blockIdx.y]) + first;
        const float ss = adam.scratch[blockIdx.y], ib = adam.scratch[kAdamGroup + blockIdx.y];
        f32x4_t p[kTrips], m[kTrips], v[kTrips];
#pragma unroll
        for (uint32_t u = 0; u < kTrips; ++u) {      // all twelve requests first (the moments stream; the parameters were gathered from by this step's encoder)
            const uint32_t i4 = threadIdx.x + u * 1024u;
            p[u] = pp[i4];
            m[u] = __builtin_nontemporal_load(pm + i4);
            v[u] = __builtin_nontemporal_load(pv + i4);
        }
#pragma unroll
        for (uint32_t u = 0; u < kTrips; ++u) {
            const uint32_t i4 = threadIdx.x + u * 1024u;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const long long a = (long long)acc64[4u * i4 + c];
                const float g = (poisoned ? __uint_as_float(0x7fc00000u) : (a != 0 ? (float)ldexp((double)a, -k) : 0.0f)) * adam.grad_scale;      // (what the plain owner stores, times opt_adam_dense's factor)
                float pe = p[u][c], me = m[u][c], ve = v[u][c];
                adam_update(g, pe, me, ve, adam.beta1, adam.beta2, adam.eps, ss, ib);
                p[u][c] = pe; m[u][c] = me; v[u][c] = ve;
            }
            pp[i4] = p[u];      // (through the caches: the next step's encoder gathers from them; the moments stream out -- k_adam_dense_v4's policy)
            __builtin_nontemporal_store(m[u], pm + i4);
            __builtin_nontemporal_store(v[u], pv + i4);
        }
        return;
    }
    if (add_to_g && !poisoned) {
        // what k_scatter_merge does with the sum of a slice's slabs, done here with the one owner's accumulators: the same integer, the same conversion, one float
        // atomic per non-zero element (consecutive lanes on consecutive words, as in the merge) -- the same bits in G, no slabs and no second launch
        for (uint32_t i = threadIdx.x; i < 2u * kBinRows; i += blockDim.x) {
            const long long v = (long long)acc64[i];
            if (v != 0) atomicAdd(out + i, (float)ldexp((double)v, -k));
        }
    } else if (poisoned || replicas == 1) {
        for (uint32_t i4 = threadIdx.x; i4 < kBinRows / 2u; i4 += blockDim.x) {      // two rows = four sums per thread and trip: 16-byte stores (the slice is 64 KiB-aligned in G)
            float r[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const long long v = (long long)acc64[4u * i4 + c];
                r[c] = poisoned ? __uint_as_float(0x7fc00000u) : (v != 0 ? (float)ldexp((double)v, -k) : 0.0f);
            }
            *reinterpret_cast<float4 *>(out + 4u * i4) = make_float4(r[0], r[1], r[2], r[3]);
        }
    } else {
        // this replica's slab for k_scatter_merge (plain 16-byte stores; the launch boundary makes them visible)
        typedef unsigned long long u64x2_t __attribute__((ext_vector_type(2)));
        constexpr uint32_t kSlab = 2u * kBinRows;
        u64x2_t *mine = reinterpret_cast<u64x2_t *>(slabs + ((size_t)blockIdx.y * kBinSlices * replicas + (size_t)slice * replicas + replica) * kSlab);
        for (uint32_t i2 = threadIdx.x; i2 < kBinRows; i2 += blockDim.x) mine[i2] = *reinterpret_cast<const u64x2_t *>(acc64 + 2u * i2);
    }
}

// The exact merge of a slice's replicas (see k_scatter_binned).  blockIdx.x = slice * kMergeParts + part: a quarter of the slice's words per workgroup, one 8-byte
// fixed-point sum per thread and trip -- consecutive lanes on consecutive words, for the loads and for the atomics behind them (an atomic wave instruction leaves
// the L2 as one request per 64 bytes it touches; a row pair per lane would double them).  The scale is the one the replicas used (fixed_scale of the launch's
// gmax and the slice's entry count); a poisoned
// launch has written its NaNs already.  One float atomic per non-zero element and launch.
constexpr uint32_t kMergeParts = 4, kMergeThreads = 1024;
__global__ void __launch_bounds__(kMergeThreads) k_scatter_merge(const BinHeader *__restrict__ hd_all, ScatterTargets tg, uint32_t replicas,
                                                                 const unsigned long long *__restrict__ slabs) {
    constexpr uint32_t kSlab = 2u * kBinRows, kPartWords = kSlab / kMergeParts, kTrips = kPartWords / kMergeThreads;
    static_assert(kPartWords % kMergeThreads == 0, "whole trips");
    const BinHeader *__restrict__ hd = hd_all + blockIdx.y;
    const uint32_t slice = blockIdx.x / kMergeParts, part = blockIdx.x - slice * kMergeParts;
    const uint32_t n = hd->counts[slice], gb = hd->gmax_bits;
    if (n == 0 || gb >= 0x7f800000u) return;      // (uniform) an empty slice; a poisoned launch
    const int k = fixed_scale(gb, n);
    const uint32_t chunk = ceil_div(n, replicas);
    const unsigned long long *slice_slabs = slabs + ((size_t)blockIdx.y * kBinSlices + slice) * replicas * kSlab + (size_t)part * kPartWords;
    unsigned long long sum[kTrips];
#pragma unroll
    for (uint32_t u = 0; u < kTrips; ++u) sum[u] = 0ull;
    for (uint32_t r = 0; r < replicas; ++r) {
        if (min(n, r * chunk) >= n) break;      // (uniform) this replica and the ones behind it had no entries and left no slab
        unsigned long long got[kTrips];
#pragma unroll
        for (uint32_t u = 0; u < kTrips; ++u) got[u] = __builtin_nontemporal_load(slice_slabs + (size_t)r * kSlab + threadIdx.x + u * kMergeThreads);
#pragma unroll
        for (uint32_t u = 0; u < kTrips; ++u) sum[u] += got[u];
    }
    float *out = tg.g[blockIdx.y] + 2 * (size_t)slice * kBinRows + (size_t)part * kPartWords;
#pragma unroll
    for (uint32_t u = 0; u < kTrips; ++u) {
        const long long v = (long long)sum[u];
        if (v != 0) atomicAdd(out + threadIdx.x + u * kMergeThreads, (float)ldexp((double)v, -k));
    }
}

// Stage-1 training scatters into all 16 base tables.  The cell index and weights of a (point, level) need the level's IEEE
// divisions (corner_rows), which the 32 slice owners of that level would each repeat: instead they are computed once here, into
// the same 32-byte record the codebook scatter consumes, and k_scatter_sliced runs over 16 record sets.
__global__ void __launch_bounds__(256) k_level_records(const float *__restrict__ xyzs, float bound, const float2 *__restrict__ dplanes, uint32_t M,
                                                       uint32_t stride, LevelGeom geom, uint4 *__restrict__ rec) {
    const uint32_t m = blockIdx.x * 256 + threadIdx.x, level = blockIdx.y;
    if (m >= M) return;
    const float2 g = dplanes[(size_t)level * stride + m];
    const float two_b = 2.0f * bound, cell = geom.cell[level];
    uint32_t idx[3];
    float w[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) axis_cell((xyzs[3 * (size_t)m + a] + bound) / two_b, cell, idx[a], w[a]);
    uint4 *r4 = rec + 2 * ((size_t)level * M + m);
    r4[0] = make_uint4(idx[0] | (idx[1] << 16), idx[2], __float_as_uint(w[0]), __float_as_uint(w[1]));
    r4[1] = make_uint4(__float_as_uint(w[2]), __float_as_uint(g.x), __float_as_uint(g.y), 0u);
}

// grads[i][e] (+)= G[e]: float4 per lane, D output streams.
__global__ void __launch_bounds__(256) k_fanout(const float4 *__restrict__ G, GradPtrs grads, uint32_t D, int accumulate) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= NSIG_TABLE_ROWS / 2) return;
    const float4 g = G[e];
    for (uint32_t i = 0; i < D; ++i) {
        float4 *dst = reinterpret_cast<float4 *>(grads.p[i]) + e;
        if (accumulate) {
            float4 v = *dst;
            v.x += g.x; v.y += g.y; v.z += g.z; v.w += g.w;
            *dst = v;
        } else *dst = g;
    }
}

__global__ void __launch_bounds__(256) k_level_lookup(const float *__restrict__ x01, uint32_t M, float cell, int32_t *__restrict__ rows,
                                                      float *__restrict__ weights) {
    const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    Corner8 c;
    corner_rows(x01[3 * (size_t)m], x01[3 * (size_t)m + 1], x01[3 * (size_t)m + 2], cell, c);
#pragma unroll
    for (int k = 0; k < 8; ++k) rows[8 * (size_t)m + k] = (int32_t)c.row[k];
    weights[3 * (size_t)m] = c.wx; weights[3 * (size_t)m + 1] = c.wy; weights[3 * (size_t)m + 2] = c.wz;
}

// ----------------------------------------------------------------------------- device-side table selection
// (every launch argument independent of the message: the enclosing step can be captured in a hipGraph)

struct PairPtrs {
    const float *p[2 * NSIG_MAX_MESSAGE_DIM];
};

__global__ void __launch_bounds__(256) k_codebook_presum_sel(PairPtrs tabs, const float *__restrict__ message, uint32_t D, float4 *__restrict__ S) {
    // Resolve the D selected tables once per workgroup (a chain message -> pointer -> data per table would otherwise sit in
    // front of every load), then stream them eight at a time.
    __shared__ const float4 *sel[NSIG_MAX_MESSAGE_DIM];
    if (threadIdx.x < D) sel[threadIdx.x] = reinterpret_cast<const float4 *>(tabs.p[2 * threadIdx.x + (message[threadIdx.x] != 0.0f)]);
    __syncthreads();
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= NSIG_TABLE_ROWS / 2) return;
    float4 acc = {0.f, 0.f, 0.f, 0.f};
    uint32_t i = 0;
    for (; i + 8 <= D; i += 8) {   // the sum keeps the table order (bit-identical to the serial sum)
        float4 t[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) t[u] = sel[i + u][e];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            acc.x += t[u].x; acc.y += t[u].y; acc.z += t[u].z; acc.w += t[u].w;
        }
    }
    for (; i < D; ++i) {
        const float4 a = sel[i][e];
        acc.x += a.x; acc.y += a.y; acc.z += a.z; acc.w += a.w;
    }
    S[e] = acc;
}

// hg_codebook_presum_multi: K messages in ONE pass over the 2 D tables.  A thread owns the same float4 (two rows) of every table as above, reads BOTH tables of
// a pair once and adds, per message, the one the message's bit names -- per message the serial sum in table order of k_codebook_presum_sel, so S_k has its bits.
// bits[i] holds bit i of every message (message k in bit k).  KC >= K accumulators (a power of two; the ones past K follow message "all zero" and are dropped).
// Output row-interleaved, S_multi[row][k] (float2): a thread's two rows are 2 K consecutive float2 -- 16-byte stores when K is even.
static_assert(NSIG_MULTI_MAX_MESSAGES == 16, "hg_codebook_presum_multi instantiates 1, 2, 4, 8 and 16 accumulators");
template <int KC>
__device__ __forceinline__ void presum_multi_add(float4 (&acc)[KC], const float4 t0, const float4 t1, const uint32_t w) {
#pragma unroll
    for (int k = 0; k < KC; ++k) {
        const bool one = ((w >> k) & 1u) != 0u;
        acc[k].x += one ? t1.x : t0.x; acc[k].y += one ? t1.y : t0.y; acc[k].z += one ? t1.z : t0.z; acc[k].w += one ? t1.w : t0.w;
    }
}

template <int KC>
__global__ void __launch_bounds__(256) k_codebook_presum_multi(PairPtrs tabs, const float *__restrict__ messages, uint32_t K, uint32_t D, float2 *__restrict__ S_multi) {
    __shared__ uint32_t bits[NSIG_MAX_MESSAGE_DIM];
    __shared__ const float4 *tab[2 * NSIG_MAX_MESSAGE_DIM];      // (as k_codebook_presum_sel: the pointers once per workgroup, not a kernel-argument lookup per load)
    if (threadIdx.x < D) {
        uint32_t w = 0;
        for (uint32_t k = 0; k < K; ++k) w |= (messages[(size_t)k * D + threadIdx.x] != 0.0f ? 1u : 0u) << k;
        bits[threadIdx.x] = w;
    }
    if (threadIdx.x < 2 * D) tab[threadIdx.x] = reinterpret_cast<const float4 *>(tabs.p[threadIdx.x]);
    __syncthreads();
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= NSIG_TABLE_ROWS / 2) return;
    float4 acc[KC];
#pragma unroll
    for (int k = 0; k < KC; ++k) acc[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    uint32_t i = 0;
    for (; i + 4 <= D; i += 4) {      // eight loads in flight, as the single pass has; the sums keep the table order
        const float4 a0 = tab[2 * i][e], a1 = tab[2 * i + 1][e], b0 = tab[2 * i + 2][e], b1 = tab[2 * i + 3][e];
        const float4 c0 = tab[2 * i + 4][e], c1 = tab[2 * i + 5][e], d0 = tab[2 * i + 6][e], d1 = tab[2 * i + 7][e];
        presum_multi_add<KC>(acc, a0, a1, bits[i]);
        presum_multi_add<KC>(acc, b0, b1, bits[i + 1]);
        presum_multi_add<KC>(acc, c0, c1, bits[i + 2]);
        presum_multi_add<KC>(acc, d0, d1, bits[i + 3]);
    }
    for (; i < D; ++i) presum_multi_add<KC>(acc, tab[2 * i][e], tab[2 * i + 1][e], bits[i]);
    float2 *out = S_multi + (size_t)2 * e * K;      // rows 2 e and 2 e + 1
    if constexpr (KC >= 2) {
        if ((K & 1u) == 0u) {
#pragma unroll
            for (int k = 0; k < KC; k += 2)
                if ((uint32_t)k < K) {
                    *reinterpret_cast<float4 *>(out + k) = make_float4(acc[k].x, acc[k].y, acc[k + 1].x, acc[k + 1].y);
                    *reinterpret_cast<float4 *>(out + K + k) = make_float4(acc[k].z, acc[k].w, acc[k + 1].z, acc[k + 1].w);
                }
            return;
        }
    }
#pragma unroll
    for (int k = 0; k < KC; ++k)
        if ((uint32_t)k < K) {
            out[k] = make_float2(acc[k].x, acc[k].y);
            out[K + k] = make_float2(acc[k].z, acc[k].w);
        }
}

}  // namespace nsig

using namespace nsig;

NSIG_EXPORT int hg_codebook_presum(const float *const *tables_host, uint32_t D, float *S, nsig_stream_t stream) {
    NSIG_REQUIRE(tables_host && S, "hg_codebook_presum: null pointer");
    NSIG_REQUIRE(D >= 1 && D <= NSIG_MAX_MESSAGE_DIM, "hg_codebook_presum: D=%u out of range [1,%d]", D, NSIG_MAX_MESSAGE_DIM);
    CodebookPtrs tabs{};
    const char *bad = "%s: table %u is null or not 16-byte aligned";
    if (int e = take_pointers({tabs.p}, {tables_host}, D, "hg_codebook_presum", bad, bad)) return e;
    NSIG_REQUIRE(aligned16(S), "hg_codebook_presum: S must be 16-byte aligned");
    k_codebook_presum<<<NSIG_TABLE_ROWS / 2 / 256, 256, 0, as_stream(stream)>>>(tabs, D, reinterpret_cast<float4 *>(S));
    return check_launch("hg_codebook_presum");
}

NSIG_EXPORT int hg_encode_fwd(const float *x01, uint32_t M, const float *const *base_tables_host, const float *S, float *feat,
                              nsig_stream_t stream) {
    if (M == 0) return NSIG_OK;
    NSIG_REQUIRE(x01 && feat, "hg_encode_fwd: null pointer");
    TablePtrs base{};
    if (int e = fill_base_tables(base_tables_host, base, "hg_encode_fwd")) return e;
    NSIG_REQUIRE(M <= (1u << 27), "hg_encode_fwd: M=%u too large", M);
    k_encode<<<ceil_div(M * 16u, 256), 256, 0, as_stream(stream)>>>(x01, M, base, make_level_geom(), S, feat);
    return check_launch("hg_encode_fwd");
}

NSIG_EXPORT int hg_codebook_encode_fwd(const float *x01, uint32_t M, const float *const *tables_host, uint32_t D, float *out,
                                       nsig_stream_t stream) {
    if (M == 0) return NSIG_OK;
    NSIG_REQUIRE(x01 && tables_host && out, "hg_codebook_encode_fwd: null pointer");
    NSIG_REQUIRE(D >= 1 && D <= NSIG_MAX_MESSAGE_DIM, "hg_codebook_encode_fwd: D=%u out of range", D);
    CodebookPtrs tabs{};
    if (int e = take_pointers({tabs.p}, {tables_host}, D, "hg_codebook_encode_fwd", "%s: table %u is null")) return e;
    k_codebook_encode<<<ceil_div(M, 256), 256, 0, as_stream(stream)>>>(x01, M, tabs, D, 1.0f / kCodebookResolution, out);
    return check_launch("hg_codebook_encode_fwd");
}

NSIG_EXPORT int hg_codebook_bwd(const float *x01, uint32_t M, const float *dfeat, float *G, nsig_stream_t stream) {
    if (M == 0) return NSIG_OK;
    NSIG_REQUIRE(x01 && dfeat && G, "hg_codebook_bwd: null pointer");
    NSIG_REQUIRE(M <= (1u << 27), "hg_codebook_bwd: M=%u too large", M);
    k_codebook_bwd<<<ceil_div(M * 16u, 256), 256, 0, as_stream(stream)>>>(x01, M, dfeat, 1.0f / kCodebookResolution, G);
    return check_launch("hg_codebook_bwd");
}

NSIG_EXPORT int hg_fanout_grad(const float *G, float *const *grads_host, uint32_t D, int accumulate, nsig_stream_t stream) {
    NSIG_REQUIRE(G && grads_host, "hg_fanout_grad: null pointer");
    NSIG_REQUIRE(D >= 1 && D <= NSIG_MAX_MESSAGE_DIM, "hg_fanout_grad: D=%u out of range", D);
    GradPtrs grads{};
    const char *bad = "%s: gradient %u is null or not 16-byte aligned";
    if (int e = take_pointers({grads.p}, {grads_host}, D, "hg_fanout_grad", bad, bad)) return e;
    NSIG_REQUIRE(aligned16(G), "hg_fanout_grad: G must be 16-byte aligned");
    k_fanout<<<NSIG_TABLE_ROWS / 2 / 256, 256, 0, as_stream(stream)>>>(reinterpret_cast<const float4 *>(G), grads, D, accumulate);
    return check_launch("hg_fanout_grad");
}

NSIG_EXPORT int hg_level_lookup(const float *x01, uint32_t M, float resolution, int32_t *rows, float *weights, nsig_stream_t stream) {
    if (M == 0) return NSIG_OK;
    NSIG_REQUIRE(x01 && rows && weights, "hg_level_lookup: null pointer");
    NSIG_REQUIRE(resolution >= 1.0f, "hg_level_lookup: resolution must be >= 1");
    k_level_lookup<<<ceil_div(M, 256), 256, 0, as_stream(stream)>>>(x01, M, 1.0f / resolution, rows, weights);
    return check_launch("hg_level_lookup");
}

NSIG_EXPORT int hg_scatter_sliced(const float *rec, uint32_t M, float *G, nsig_stream_t stream) {
    if (M == 0) return NSIG_OK;
    NSIG_REQUIRE(rec && G, "hg_scatter_sliced: null pointer");
    static std::atomic<size_t> granted{0};
    const size_t lds = (size_t)kSliceRows * 2 * sizeof(float);
    if (int e = reserve_lds(k_scatter_sliced, lds, granted, "hg_scatter_sliced")) return e;
    ScatterTargets tg{};
    tg.g[0] = G;
    k_scatter_sliced<<<kSlices * kReplicas, 1024, lds, as_stream(stream)>>>(rec, M, tg, 1u, (uint32_t)kReplicas);
    return check_launch("hg_scatter_sliced");
}

NSIG_EXPORT int hg_codebook_presum_sel(const float *const *all_tables_host, const float *message, uint32_t D, float *S, nsig_stream_t stream) {
    NSIG_REQUIRE(all_tables_host && message && S, "hg_codebook_presum_sel: null pointer");
    NSIG_REQUIRE(D >= 1 && D <= NSIG_MAX_MESSAGE_DIM, "hg_codebook_presum_sel: D=%u out of range [1,%d]", D, NSIG_MAX_MESSAGE_DIM);
    PairPtrs tabs{};
    const char *bad = "%s: table %u is null or not 16-byte aligned";
    if (int e = take_pointers({tabs.p}, {all_tables_host}, 2 * D, "hg_codebook_presum_sel", bad, bad)) return e;
    NSIG_REQUIRE(aligned16(S), "hg_codebook_presum_sel: S must be 16-byte aligned");
    k_codebook_presum_sel<<<NSIG_TABLE_ROWS / 2 / 256, 256, 0, as_stream(stream)>>>(tabs, message, D, reinterpret_cast<float4 *>(S));
    return check_launch("hg_codebook_presum_sel");
}

NSIG_EXPORT size_t hg_multi_presum_bytes(uint32_t K) { return (size_t)K * NSIG_TABLE_ROWS * sizeof(float2); }

NSIG_EXPORT int hg_codebook_presum_multi(const float *const *all_tables_host, const float *messages, uint32_t K, uint32_t D, void *S_multi, nsig_stream_t stream) {
    NSIG_REQUIRE(all_tables_host && messages && S_multi, "hg_codebook_presum_multi: null pointer");
    NSIG_REQUIRE(K >= 1 && K <= NSIG_MULTI_MAX_MESSAGES, "hg_codebook_presum_multi: K=%u out of range [1,%d]", K, NSIG_MULTI_MAX_MESSAGES);
    NSIG_REQUIRE(D >= 1 && D <= NSIG_MAX_MESSAGE_DIM, "hg_codebook_presum_multi: D=%u out of range [1,%d]", D, NSIG_MAX_MESSAGE_DIM);
    PairPtrs tabs{};
    const char *bad = "%s: table %u is null or not 16-byte aligned";
    if (int e = take_pointers({tabs.p}, {all_tables_host}, 2 * D, "hg_codebook_presum_multi", bad, bad)) return e;
    NSIG_REQUIRE(aligned16(S_multi), "hg_codebook_presum_multi: S_multi must be 16-byte aligned");
    float2 *out = reinterpret_cast<float2 *>(S_multi);
    const dim3 grid(NSIG_TABLE_ROWS / 2 / 256);
    hipStream_t st = as_stream(stream);
    if (K == 1) k_codebook_presum_multi<1><<<grid, 256, 0, st>>>(tabs, messages, K, D, out);
    else if (K == 2) k_codebook_presum_multi<2><<<grid, 256, 0, st>>>(tabs, messages, K, D, out);
    else if (K <= 4) k_codebook_presum_multi<4><<<grid, 256, 0, st>>>(tabs, messages, K, D, out);
    else if (K <= 8) k_codebook_presum_multi<8><<<grid, 256, 0, st>>>(tabs, messages, K, D, out);
    else k_codebook_presum_multi<16><<<grid, 256, 0, st>>>(tabs, messages, K, D, out);
    return check_launch("hg_codebook_presum_multi");
}

// no points: the 16 gradient tables of a level scatter are all zeros
static int zero_level_tables(const ScatterTargets &tg, hipStream_t st, const char *who) {
    for (int l = 0; l < NSIG_BASE_LEVELS; ++l)
        if (hipMemsetAsync(tg.g[l], 0, (size_t)NSIG_TABLE_ROWS * 2 * sizeof(float), st) != hipSuccess) {
            set_error("%s: hipMemsetAsync failed", who);
            return NSIG_ERR_LAUNCH;
        }
    return NSIG_OK;
}

static size_t binned_scratch_bytes(uint32_t M, uint32_t sets) { return (size_t)sets * (sizeof(BinHeader) + (size_t)4 * M * sizeof(uint4)); }

static int reserve_owner_lds(const char *who) {
    static std::atomic<size_t> granted{0};
    return reserve_lds(k_scatter_binned, (size_t)kBinRows * 2 * sizeof(unsigned long long), granted, who);
}

// sets record arrays [sets][M][8] -> sets tables; scratch = sets headers, then sets queues
// the owners store their rows as 16-byte vectors
static int owner_targets_aligned(const ScatterTargets &tg, uint32_t sets, const char *who) {
    for (uint32_t i = 0; i < sets; ++i) NSIG_REQUIRE(aligned16(tg.g[i]), "%s: gradient table %u must be 16-byte aligned", who, i);
    return NSIG_OK;
}

static int launch_binned(const float *rec, uint32_t M, uint32_t sets, const ScatterTargets &tg, uint32_t replicas, void *scratch, hipStream_t st,
                         const char *who) {
    static_assert(sizeof(BinHeader) % 16 == 0 && kBinGrid == 16 * 16, "the queues follow the headers 16-byte aligned; k_bin_scan walks 16 x 16 workgroups");
    BinHeader *hd = reinterpret_cast<BinHeader *>(scratch);
    uint4 *queue = reinterpret_cast<uint4 *>(hd + sets);
    for (uint32_t i = 0; i < sets; ++i)
        if (hipMemsetAsync(&hd[i].gmax_bits, 0, sizeof(uint32_t), st) != hipSuccess) {
            set_error("%s: hipMemsetAsync failed", who);
            return NSIG_ERR_LAUNCH;
        }
    const size_t lds = (size_t)kBinRows * 2 * sizeof(unsigned long long);
    if (int e = reserve_owner_lds(who)) return e;
    if (int e = owner_targets_aligned(tg, sets, who)) return e;
    const uint32_t blocks = ceil_div(M, kBinThreads) < kBinGrid ? ceil_div(M, kBinThreads) : kBinGrid;
    k_bin_count<<<dim3(blocks, sets), kBinThreads, 0, st>>>(rec, M, hd);
    k_bin_scan<<<sets, 1024, 0, st>>>(hd, blocks);
    k_bin_write<<<dim3(blocks, sets), kBinThreads, 0, st>>>(rec, M, hd, queue);
    unsigned long long *slabs = replicas > 1 ? reinterpret_cast<unsigned long long *>(queue + (size_t)sets * 4 * M) : nullptr;      // (the merge scratch follows the queues)
    k_scatter_binned<<<dim3(kBinSlices * replicas, sets), 1024, lds, st>>>(hd, queue, M, tg, replicas, nullptr, 0u, OwnerAdam{}, slabs);
    if (replicas > 1) k_scatter_merge<<<dim3(kBinSlices * kMergeParts, sets), kMergeThreads, 0, st>>>(hd, tg, replicas, slabs);
    return check_launch(who);
}

NSIG_EXPORT size_t hg_scatter_binned_scratch_bytes(uint32_t M) { return binned_scratch_bytes(M, 1) + scatter_merge_bytes(kBinReplicas); }

NSIG_EXPORT int hg_scatter_binned(const float *rec, uint32_t M, float *G, void *scratch, nsig_stream_t stream) {
    if (M == 0) return NSIG_OK;
    NSIG_REQUIRE(rec && G && scratch, "hg_scatter_binned: null pointer");
    NSIG_REQUIRE(aligned16(rec) && aligned16(scratch) && M < (1u << 28),
                 "hg_scatter_binned: rec and scratch must be 16-byte aligned and M < 2^28");
    ScatterTargets tg{};
    tg.g[0] = G;
    return launch_binned(rec, M, 1, tg, kBinReplicas, scratch, as_stream(stream), "hg_scatter_binned");
}

NSIG_EXPORT size_t hg_scatter_plan_bytes(uint32_t M) { return scatter_plan_bytes(M); }

// M sizes the launch and addresses the plan; rows_dev (hg_scatter_plan_rows): the kernels stop at min(M, *rows_dev)
static int scatter_plan_launch(const char *who, const float *xyzs, uint32_t M, const uint32_t *rows_dev, float bound, void *plan, nsig_stream_t stream) {
    if (M == 0) return NSIG_OK;
    NSIG_REQUIRE(xyzs && plan, "%s: null pointer", who);
    NSIG_REQUIRE(aligned16(plan) && M < (1u << 28) && bound > 0.0f, "%s: plan must be 16-byte aligned, M < 2^28, bound > 0", who);
    const ScatterPlan pl = scatter_plan_view(plan, M);
    hipStream_t st = as_stream(stream);
    const uint32_t blocks = ceil_div(M, kBinThreads) < kBinGrid ? ceil_div(M, kBinThreads) : kBinGrid;
    k_plan_count<<<blocks, kBinThreads, 0, st>>>(xyzs, M, bound, pl.hd, rows_dev);
    k_plan_dest<<<blocks, kBinThreads, 0, st>>>(xyzs, M, bound, pl.hd, pl.dest, rows_dev);
    return check_launch(who);
}

NSIG_EXPORT int hg_scatter_plan(const float *xyzs, uint32_t M, float bound, void *plan, nsig_stream_t stream) {
    return scatter_plan_launch("hg_scatter_plan", xyzs, M, nullptr, bound, plan, stream);
}

NSIG_EXPORT int hg_scatter_plan_rows(const float *xyzs, uint32_t M_capacity, const uint32_t *rows_dev, float bound, void *plan, nsig_stream_t stream) {
    NSIG_REQUIRE(rows_dev != nullptr, "hg_scatter_plan_rows: null row count");
    return scatter_plan_launch("hg_scatter_plan_rows", xyzs, M_capacity, rows_dev, bound, plan, stream);
}

// Launches of at most this many points (capacity: 4 entries each) get ONE owner per slice, which adds its rows to G itself (k_scatter_binned's add_to_g): no
// slabs, no merge launch.  Same bits as the replicas + merge.  Same-box sweep of the two forms over the launch size (tools/scatter_owner_sweep.py, us per call,
// single | replicas + merge): 66 k points 10.9 | 20.4, 115 k 12.4 | 20.7, 144 k 13.3 | 20.9, 200 k 15.0 | 21.9, 288 k 17.6 | 23.1, 400 k 21.0 | 24.2,
// 576 k 26.0 | 26.3, 800 k 32.7 | 28.5, 1.29 M 46.8 | 34.4 (profiles/scatter_rows_owner_sweep.txt): the last size at which one owner is clearly ahead.
constexpr uint32_t kSingleOwnerMaxPoints = NSIG_SINGLE_OWNER_MAX_POINTS;

// owners: NSIG_OWNERS_BY_SIZE, or one of the two forms by name (the parity tests and the sweep run both on one queue)
static int scatter_planned_launch(const char *who, const void *plan, uint32_t M, float *G, int owners, nsig_stream_t stream) {
    if (M == 0) return NSIG_OK;
    NSIG_REQUIRE(plan && G, "%s: null pointer", who);
    NSIG_REQUIRE(aligned16(plan) && M < (1u << 28), "%s: plan must be 16-byte aligned and M < 2^28", who);
    NSIG_REQUIRE(owners == NSIG_OWNERS_BY_SIZE || owners == NSIG_OWNERS_SINGLE || owners == NSIG_OWNERS_REPLICAS, "%s: owners=%d is none of NSIG_OWNERS_*", who, owners);
    if (int e = reserve_owner_lds(who)) return e;
    const ScatterPlan pl = scatter_plan_view(const_cast<void *>(plan), M);
    ScatterTargets tg{};
    tg.g[0] = G;
    if (int e = owner_targets_aligned(tg, 1, who)) return e;
    hipStream_t st = as_stream(stream);
    const size_t lds = (size_t)kBinRows * 2 * sizeof(unsigned long long);
    if (owners == NSIG_OWNERS_SINGLE || (owners == NSIG_OWNERS_BY_SIZE && M <= kSingleOwnerMaxPoints)) {
        k_scatter_binned<<<dim3(kBinSlices, 1), 1024, lds, st>>>(pl.hd, pl.queue, M, tg, 1u, nullptr, 0u, OwnerAdam{}, nullptr, true);
        return check_launch(who);
    }
    // replicas: 1 -> 63 us, 2 -> 40, 4 -> 32, 8 -> 43 on 5.2 M entries (more owners stream less each, but merge with more float atomics)
    // (with the owners' pipelined queue walk, round 5: 2 -> 31.0, 3 -> 28.5, 4 -> 28.9, 6 -> 37.4, 8 -> 43.2 us; the step the same for 2..4)
    k_scatter_binned<<<dim3(kBinSlices * kBinReplicas, 1), 1024, lds, st>>>(pl.hd, pl.queue, M, tg, kBinReplicas, nullptr, 0u, OwnerAdam{}, pl.slabs);
    k_scatter_merge<<<dim3(kBinSlices * kMergeParts, 1), kMergeThreads, 0, st>>>(pl.hd, tg, kBinReplicas, pl.slabs);
    return check_launch(who);
}

NSIG_EXPORT int hg_scatter_planned(const void *plan, uint32_t M, float *G, nsig_stream_t stream) {
    return scatter_planned_launch("hg_scatter_planned", plan, M, G, NSIG_OWNERS_BY_SIZE, stream);
}

// (the owners take their entry counts from the header hg_scatter_plan_rows left: nothing in them reads the row count)
NSIG_EXPORT int hg_scatter_planned_rows(const void *plan, uint32_t M_capacity, const uint32_t *rows_dev, float *G, int owners, nsig_stream_t stream) {
    NSIG_REQUIRE(rows_dev != nullptr, "hg_scatter_planned_rows: null row count");
    return scatter_planned_launch("hg_scatter_planned_rows", plan, M_capacity, G, owners, stream);
}

NSIG_EXPORT size_t hg_scatter_levels_scratch_bytes(uint32_t M) {
    return (size_t)NSIG_BASE_LEVELS * M * 32 + binned_scratch_bytes(M, NSIG_BASE_LEVELS);   // the 16 record arrays, then the binning scratch
}

NSIG_EXPORT int hg_scatter_levels(const float *xyzs, float bound, const void *d_planes, uint32_t M, uint32_t stride, float *const *G_host,
                                  void *scratch, nsig_stream_t stream) {
    NSIG_REQUIRE(xyzs && d_planes && G_host && scratch, "hg_scatter_levels: null pointer");
    NSIG_REQUIRE(bound > 0.0f && stride >= M && M < (1u << 28), "hg_scatter_levels: bad bound, stride < M or M >= 2^28");
    NSIG_REQUIRE(aligned16(scratch), "hg_scatter_levels: scratch must be 16-byte aligned");
    ScatterTargets tg{};
    if (int e = take_pointers({tg.g}, {G_host}, NSIG_BASE_LEVELS, "hg_scatter_levels", "%s: table %u has a null pointer")) return e;
    hipStream_t st = as_stream(stream);
    if (M == 0) return zero_level_tables(tg, st, "hg_scatter_levels");
    uint4 *rec = reinterpret_cast<uint4 *>(scratch);
    k_level_records<<<dim3(ceil_div(M, 256u), NSIG_BASE_LEVELS), 256, 0, st>>>(xyzs, bound, reinterpret_cast<const float2 *>(d_planes), M, stride,
                                                                              make_level_geom(), rec);
    if (int e = check_launch("hg_scatter_levels (records)")) return e;
    // every (level, slice) has a single owner, which stores its rows: the tables are written, not accumulated into
    return launch_binned(reinterpret_cast<const float *>(rec), M, NSIG_BASE_LEVELS, tg, 1u,
                         reinterpret_cast<char *>(scratch) + (size_t)NSIG_BASE_LEVELS * M * 32, st, "hg_scatter_levels");
}

NSIG_EXPORT size_t hg_levels_plan_bytes(uint32_t M) { return levels_plan_bytes(M); }

NSIG_EXPORT int hg_levels_plan(const float *xyzs, uint32_t M, const uint32_t *rows_dev, float bound, void *plan, nsig_stream_t stream) {
    if (M == 0) return NSIG_OK;
    NSIG_REQUIRE(xyzs && plan, "hg_levels_plan: null pointer");
    NSIG_REQUIRE(aligned16(plan) && M < (1u << 27) && bound > 0.0f, "hg_levels_plan: plan must be 16-byte aligned, M < 2^27, bound > 0");
    const LevelsPlan pl = levels_plan_view(plan, M);
    hipStream_t st = as_stream(stream);
    k_levels_count<<<dim3(pl.n_chunks, NSIG_BASE_LEVELS), kBinThreads, 0, st>>>(xyzs, M, rows_dev, bound, make_level_geom(), pl);
    k_levels_scan<<<NSIG_BASE_LEVELS, kBinThreads, 0, st>>>(M, rows_dev, pl);
    return check_launch("hg_levels_plan");
}

// entries + owners of the planned 16-level scatter; adam.on: the owners end with the optimiser step of their rows instead of storing them (tg unused)
// `prepare` (optional): launched between the entries pass and the owners -- behind everything that can fail without a launch (argument checks, the LDS reservations) and
// behind the first launch: hg_levels_scatter_adam's step-count increment then never happens without the owners' update that goes with it.
template <typename Prepare>
static int levels_scatter_launch(const char *who, const float *xyzs, uint32_t M, const uint32_t *rows_dev, float bound, const void *d_planes, uint32_t stride, void *plan,
                                 const ScatterTargets &tg, const OwnerAdam &adam, hipStream_t st, Prepare prepare) {
    NSIG_REQUIRE(xyzs && d_planes && plan, "%s: null pointer", who);
    NSIG_REQUIRE(aligned16(plan) && aligned8(d_planes) && M < (1u << 27) && bound > 0.0f && stride >= M,
                 "%s: plan must be 16-byte and d_planes 8-byte aligned, M < 2^27, bound > 0, stride >= M", who);
    if (!adam.on)
        if (int e = owner_targets_aligned(tg, NSIG_BASE_LEVELS, who)) return e;
    if (int e = reserve_owner_lds(who)) return e;
    const size_t staging = (size_t)kLevelStage * sizeof(uint4);
    static std::atomic<size_t> granted{0};
    if (int e = reserve_lds(k_level_entries, staging, granted, who)) return e;
    const LevelsPlan pl = levels_plan_view(plan, M);
    k_level_entries<<<dim3(pl.n_chunks, NSIG_BASE_LEVELS), kBinThreads, staging, st>>>(xyzs, M, rows_dev, bound, reinterpret_cast<const float2 *>(d_planes), stride,
                                                                                     make_level_geom(), pl);
    if (int e = check_launch(who)) return e;
    if (int e = prepare()) return e;
    // every (level, slice) has a single owner, which stores its rows: the tables are written, not accumulated into.  (The owners address set l's
    // queue at l * 4 * M' entries: M' = 2 M is this plan's stride of 8 M.)
    const uint32_t M_stride = M * (kLevelQueueStride / 4);
#ifdef NSIG_LEVELS_SPLIT      // diagnostic build (tools/build_variant.sh): one owner launch per level, so that a kernel trace shows each level's time (the plain owners only)
    for (int l = 0; l < NSIG_BASE_LEVELS; ++l) {
        ScatterTargets one{};
        one.g[0] = tg.g[l];
        k_scatter_binned<<<dim3(kBinSlices, 1), 1024, (size_t)kBinRows * 2 * sizeof(unsigned long long), st>>>(pl.hd + l, pl.queue + (size_t)l * kLevelQueueStride * M,
                                                                                                               M_stride, one, 1u, pl.chunk_max + (size_t)l * pl.n_chunks, pl.n_chunks);
    }
#else
    k_scatter_binned<<<dim3(kBinSlices, NSIG_BASE_LEVELS), 1024, (size_t)kBinRows * 2 * sizeof(unsigned long long), st>>>(pl.hd, pl.queue, M_stride, tg, 1u,
                                                                                                                          pl.chunk_max, pl.n_chunks, adam);
#endif
    return check_launch(who);
}

NSIG_EXPORT int hg_levels_scatter(const float *xyzs, uint32_t M, const uint32_t *rows_dev, float bound, const void *d_planes, uint32_t stride, void *plan,
                                  float *const *G_host, nsig_stream_t stream) {
    NSIG_REQUIRE(G_host, "hg_levels_scatter: null pointer");
    ScatterTargets tg{};
    if (int e = take_pointers({tg.g}, {G_host}, NSIG_BASE_LEVELS, "hg_levels_scatter", "%s: table %u has a null pointer")) return e;
    hipStream_t st = as_stream(stream);
    if (M == 0) return zero_level_tables(tg, st, "hg_levels_scatter");
    return levels_scatter_launch("hg_levels_scatter", xyzs, M, rows_dev, bound, d_planes, stride, plan, tg, OwnerAdam{}, st, []() { return (int)NSIG_OK; });
}

NSIG_EXPORT int hg_levels_scatter_adam(const float *xyzs, uint32_t M, const uint32_t *rows_dev, float bound, const void *d_planes, uint32_t stride, void *plan,
                                       float *const *params_host, float *const *exp_avg_host, float *const *exp_avg_sq_host, float *const *steps_host, const float *lr,
                                       float beta1, float beta2, float eps, float grad_scale, float *scratch, nsig_stream_t stream) {
    NSIG_REQUIRE(params_host && exp_avg_host && exp_avg_sq_host && steps_host && lr && scratch, "hg_levels_scatter_adam: null pointer");
    NSIG_REQUIRE(M >= 1, "hg_levels_scatter_adam: M must be positive (a step without points still runs the owners: the device row count may be zero)");
    NSIG_REQUIRE(xyzs && d_planes && plan, "hg_levels_scatter_adam: null pointer");
    NSIG_REQUIRE(aligned16(plan) && aligned8(d_planes) && M < (1u << 27) && bound > 0.0f && stride >= M,
                 "hg_levels_scatter_adam: plan must be 16-byte and d_planes 8-byte aligned, M < 2^27, bound > 0, stride >= M");      // (before the step counts are touched)
    static_assert(NSIG_BASE_LEVELS <= kAdamGroup, "one group of the prepare launch");
    OwnerAdam adam{};
    float *steps[NSIG_BASE_LEVELS];
    if (int e = take_pointers({adam.p, adam.m, adam.v, steps}, {params_host, exp_avg_host, exp_avg_sq_host, steps_host}, NSIG_BASE_LEVELS, "hg_levels_scatter_adam",
                              "%s: table %u has a null pointer", "%s: table %u must be 16-byte aligned", 3)) return e;
    adam.scratch = scratch;
    adam.beta1 = beta1; adam.beta2 = beta2; adam.eps = eps; adam.grad_scale = grad_scale;
    adam.on = 1u;
    hipStream_t st = as_stream(stream);
    return levels_scatter_launch("hg_levels_scatter_adam", xyzs, M, rows_dev, bound, d_planes, stride, plan, ScatterTargets{}, adam, st, [&]() {      // step counts + 1, the two scalars per table
        return adam_prepare_launch(steps, NSIG_BASE_LEVELS, lr, beta1, beta2, scratch, st, "hg_levels_scatter_adam (prepare)");
    });
}

NSIG_EXPORT int hg_scatter_level(const float *xyzs, float bound, const void *d_plane, uint32_t M, uint32_t level, float *G, nsig_stream_t stream) {
    if (M == 0) return NSIG_OK;
    NSIG_REQUIRE(xyzs && d_plane && G, "hg_scatter_level: null pointer");
    NSIG_REQUIRE(level < NSIG_BASE_LEVELS && bound > 0.0f, "hg_scatter_level: level %u out of range or bad bound", level);
    static std::atomic<size_t> granted{0};
    const size_t lds = (size_t)kSliceRows * 2 * sizeof(float);
    if (int e = reserve_lds(k_scatter_level, lds, granted, "hg_scatter_level")) return e;
    k_scatter_level<<<kSlices * kReplicas, 1024, lds, as_stream(stream)>>>(xyzs, bound, reinterpret_cast<const float2 *>(d_plane), M,
                                                                         1.0f / kBaseResolution[level], G);
    return check_launch("hg_scatter_level");
}
