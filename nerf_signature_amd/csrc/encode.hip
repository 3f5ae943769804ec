// XCD-partitioned, level-major hash-grid encoder for gfx950: points -> a plane set (planes.h) that the MLP kernels of field.hip read.
//
// Behavioural reference: network_wtmk_tcnn.py:97-106 (the encoder half of NeRFNetwork.density), lookup arithmetic in hashgrid.h.
//
// The expensive part of the encoder is the 5-6 finest levels: consecutive
// points of a ray fall into different cells there, so every point costs ~4 distinct cache lines per level, served from
// beyond L2 when all 17 tables (68 MiB) compete for each XCD's 4 MiB L2.  Workgroups are dealt round-robin over the 8
// XCDs (blockIdx % 8 labels the XCD group; a speed assumption only), so workgroup (tile, slot = blockIdx % 8) encodes
// for its tile of 256 points only the levels assigned to that slot: each XCD then gathers from ONE fine table (4 MiB,
// L2-sized) plus a few coarse ones.  Features are written level-major, planes[level][point] (float2), so the stores of
// a wave are 512 contiguous bytes; streaming loads/stores are non-temporal to leave L2 to the tables.
#include "hashgrid.h"
#include "packed.h"
#include "planes.h"

namespace nsig {

struct SlotTable {
    uint8_t n[8];
    uint8_t level[8][8];      // 0..15 base levels, 16 = pre-summed codebook; every level belongs to exactly one slot
};

// Lane pairs cooperate on the gathers.  A gather costs ~2.4 clk per distinct 128-byte line per instruction plus ~1 clk per lane
// (tools/micro/gather_rate.hip), and the two x-neighbours of a (dy, dz) pair share a line in 15 of 16 cells.  With one lane per
// point they sit in two different instructions (64 lines each: one misses L1, the next hits it); here lanes 2i and 2i+1 first
// fetch the x = 0 / x = 1 sides of point 2i, then of point 2i+1, so every instruction touches 32 lines instead of 64 and none
// relies on L1 to keep a line until its partner instruction arrives.  Same number of gather instructions, same values; the
// cell hashes travel from the owner to its neighbour by DPP, the fetched corners back the same way.
__device__ inline uint32_t dpp_u(uint32_t v, int ctrl) {
    switch (ctrl) {   // quad_perm selectors must be immediates
        case 0: return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xA0, 0xF, 0xF, true);    // [0,0,2,2]: the even lane's value
        case 1: return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xF5, 0xF, 0xF, true);    // [1,1,3,3]: the odd lane's value
        default: return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, true);   // [1,0,3,2]: swap with the neighbour
    }
}

// A row source: one table as the gather sees it -- what a row word is, how to load it, how a lane hands it to its neighbour, how to decode it.
// fp32 table: the word is the float2 row itself.
struct F32Rows {
    typedef float2 Word;
    const float2 *table;
    __device__ Word load(uint32_t row) const { return table[row]; }
    __device__ static Word swap(Word w) { return make_float2(__uint_as_float(dpp_u(__float_as_uint(w.x), 2)), __uint_as_float(dpp_u(__float_as_uint(w.y), 2))); }
    __device__ float2 decode(Word w) const { return w; }
};
// Packed table (formats and decode: include/nerfsig.h "packed released model", packed.h): the word is the raw 4-, 2- or 1-byte row.  The lane pair exchanges the RAW
// words (one exchange per corner instead of two) and every lane decodes the eight corners of its own point once; decode(word) is a pure function of the word, so the
// floats are those the fp32 source gathers from the decoded table.
template <int FMT>
struct PackedRows {
    typedef uint32_t Word;
    const void *table;
    float lo, step;
    __device__ Word load(uint32_t row) const { return pk_load_row<FMT>(table, row); }      // (a row index is < NSIG_TABLE_ROWS: inside the table's pk_table_bytes)
    __device__ static Word swap(Word w) { return dpp_u(w, 2); }
    __device__ float2 decode(Word w) const { return pk_decode_row<FMT>(w, lo, step); }
};

// One level of one 256-point tile: lane pairs fetch the two x sides (see above), trilinear interpolation, one streaming store.
template <typename Rows>
__device__ inline void encode_tile_level(const Rows &rows, float cell, uint32_t xs, float3 p, float2 *__restrict__ out, bool half_out = false, bool streaming = true) {
    uint32_t ix, iy, iz;
    float wx, wy, wz;
    axis_cell(p.x, cell, ix, wx);
    axis_cell(p.y, cell, iy, wy);
    axis_cell(p.z, cell, iz, wz);
    const uint32_t hy0 = iy * kPrimeY, hy1 = (iy + 1u) * kPrimeY, hz0 = iz * kPrimeZ, hz1 = (iz + 1u) * kPrimeZ;   // corner_rows()
    typename Rows::Word v[2][4];   // v[P][q]: this lane's x side of point P of the pair, corner (dy, dz) = (q >> 1, q & 1)
#pragma unroll
    for (int P = 0; P < 2; ++P) {
        const uint32_t hx = dpp_u(ix, P) + xs;
        const uint32_t a0 = dpp_u(hy0, P), a1 = dpp_u(hy1, P), b0 = dpp_u(hz0, P), b1 = dpp_u(hz1, P);
        v[P][0] = rows.load((hx ^ a0 ^ b0) & kRowMask);
        v[P][1] = rows.load((hx ^ a0 ^ b1) & kRowMask);
        v[P][2] = rows.load((hx ^ a1 ^ b0) & kRowMask);
        v[P][3] = rows.load((hx ^ a1 ^ b1) & kRowMask);
    }
    float2 e[8];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const typename Rows::Word mine = xs ? v[1][q] : v[0][q];      // my own point, my x side
        const typename Rows::Word give = xs ? v[0][q] : v[1][q];      // the neighbour's point, my x side
        const typename Rows::Word got = Rows::swap(give);             // my own point, the other x side (fetched by the neighbour)
        e[q] = rows.decode(xs ? got : mine);          // corner k = 4*dx + q
        e[4 + q] = rows.decode(xs ? mine : got);
    }
    const float2 val = trilerp(e, wx, wy, wz);
    if (half_out) {      // (a level of a mixed plane set: `out` addresses 4-byte elements)
        __builtin_nontemporal_store(cvt_pk_f16(val.x, val.y), reinterpret_cast<uint32_t *>(out));
        return;
    }
    const f32x2 vv = {val.x, val.y};
    // the all-fp32 plane set (stage 1, the split-bf16 MLP) goes through the caches: its consumer runs right behind this launch and found the planes in memory when
    // they were streamed out (stage-1 forward 166 -> 133 us, this launch +2.5, same box, two rounds); the mixed set of the headline step keeps its streaming
    // stores (LABNOTES section 12: fewer store transactions on the fabric the line fills compete for)
    if (streaming) __builtin_nontemporal_store(vv, reinterpret_cast<f32x2 *>(out));
    else *reinterpret_cast<f32x2 *>(out) = vv;
}

// Row `row` of xyzs in the unit cube (network_wtmk_tcnn.py:101), one 12-byte load: the encoder is bound by the address path, every instruction counts.
__device__ inline float3 unit_point(const float *__restrict__ xyzs, uint32_t row, float bound) {
    const float two_b = 2.0f * bound;
    const float3 pt = *reinterpret_cast<const float3 *>(xyzs + 3 * (size_t)row);
    return make_float3((pt.x + bound) / two_b, (pt.y + bound) / two_b, (pt.z + bound) / two_b);
}

// Reads a slot's finest table (its first) through that slot's XCD (blockIdx % 8): its L2 then holds that table when the encoder starts.  Only that one: it is the
// L2's size, and the slot's coarser tables behind it made the pass as long as the fullest slot's 12 MiB (include/nerfsig.h, hg_warm_tables).
__global__ void __launch_bounds__(256) k_warm_tables(TablePtrs base, const float *__restrict__ S, SlotTable tab, float *__restrict__ sink) {
    const uint32_t slot = blockIdx.x & 7u, wg = blockIdx.x >> 3, n_wg = gridDim.x >> 3;
    float acc = 0.0f;
    if (tab.n[slot] > 0) {
        const int l = tab.level[slot][0];
        const float4 *t = reinterpret_cast<const float4 *>(l == NSIG_BASE_LEVELS ? S : base.p[l]);
        // eight requests per lane before the first is waited for (the default grid: all of a lane's eight): one at a time, the pass was eight memory latencies long
        for (uint32_t e = wg * 256 + threadIdx.x; t != nullptr && e < NSIG_TABLE_ROWS / 2; e += 8 * n_wg * 256) {
            float4 v[8];
#pragma unroll
            for (uint32_t k = 0; k < 8; ++k) v[k] = t[min(e + k * n_wg * 256, NSIG_TABLE_ROWS / 2 - 1)];
#pragma unroll
            for (uint32_t k = 0; k < 8; ++k) acc += v[k].x + v[k].y + v[k].z + v[k].w;
        }
    }
    if (acc == 1.2345e-33f) *sink = acc;      // (never: keeps the loads)
}

// The tables of a launch: level l's row source.  fp32: the 16 base tables and the pre-summed codebook S (level 16, NULL without one).
struct F32Tables {
    TablePtrs base;
    const float *S;
    bool has_codebook() const { return S != nullptr; }
    __device__ F32Rows rows(int l) const { return F32Rows{reinterpret_cast<const float2 *>(l == NSIG_BASE_LEVELS ? S : base.p[l])}; }
};
// packed: 17 tables of one format ([16]: the signature table, NULL without one); params[l] = {lo, step} of table l
template <int FMT>
struct PackedTables {
    const void *p[NSIG_BASE_LEVELS + 1];
    const float2 *params;
    bool has_codebook() const { return p[NSIG_BASE_LEVELS] != nullptr; }
    __device__ PackedRows<FMT> rows(int l) const {
        f32x2 ps = {0.0f, 0.0f};
        // uniform: one scalar load per level.  Read through the constant address space -- the parameters are written before the launch, never during it -- because a
        // pointer inside a kernel argument cannot be __restrict__, and behind the previous level's store the load would otherwise be a vector load.
        typedef const f32x2 __attribute__((address_space(4))) *ConstParams;
        if (FMT != NSIG_PACK_F16) ps = reinterpret_cast<ConstParams>(reinterpret_cast<uintptr_t>(params))[l];
        return PackedRows<FMT>{p[l], ps[0], ps[1]};
    }
};

// Workgroup (tile, slot) encodes, for its 256 points, the levels assigned to its XCD slot.
// (the plane layout as a compile-time constant: the destination of a level's features is then one address computation, not a chain of branches per level)
template <typename Tables, bool mixed>
__global__ void __launch_bounds__(256) k_encode_planes(const float *__restrict__ xyzs, uint32_t M, float bound, Tables tables, LevelGeom geom, float2 *__restrict__ planes,
                                                       uint32_t stride, SlotTable tab, const uint32_t *__restrict__ rows_dev) {
    // rows_dev (the eval loop's bursts, hg_encode_planes_rows): the number of rows that exist is known on the device only; the launch is sized for `M`
    // (the buffers' capacity, which also fixes the plane stride) and rows beyond the count are skipped
    uint32_t lim = stride;
    if (rows_dev != nullptr) {
        const uint32_t r = *rows_dev;
        if (r == 0) return;
        M = min(M, r);
        lim = min(stride, plane_stride(M));
    }
    const uint32_t slot = blockIdx.x & 7u;
    const uint32_t n_tiles = ceil_div(stride, 256u);
    const int n_levels = tab.n[slot];
    const uint32_t xs = threadIdx.x & 1u;   // which x side of the cell this lane fetches
    for (uint32_t tile = blockIdx.x >> 3; tile < n_tiles; tile += gridDim.x >> 3) {
        const uint32_t m = tile * 256 + threadIdx.x;
        if (m >= lim) continue;             // a multiple of 32: lane pairs (and DPP quads) are in or out together
        const float3 p = unit_point(xyzs, min(m, M - 1), bound);      // rows in [M, stride) replicate the last point (never consumed)
        for (int i = 0; i < n_levels; ++i) {
            const int l = tab.level[slot][i];
            float2 *out = plane_dest(planes, stride, mixed, l, m);      // (a statement of its own, in front of rows(l): behind the parameter load its address arithmetic cost the q8 / q4 launches 0.3-1.2 %)
            encode_tile_level(tables.rows(l), geom.cell[l], xs, p, out, mixed && l < kHalfLevels, /*streaming=*/mixed);
        }
    }
}

// The codebook level alone, into plane 16 of a plane set whose base planes are already there (hg_encode_codebook_plane: rays that
// do not change between steps).  One tile per workgroup, all XCDs: S (4 MiB) is the only table, every L2 holds its own copy.
// reset: the header of a scatter plan kept across steps -- its largest-gradient word starts every step at zero (k_plan_dest does
// that for a plan computed per step).
__global__ void __launch_bounds__(256) k_encode_codebook_plane(const float *__restrict__ xyzs, uint32_t M, float bound, float cell, const float *__restrict__ S,
                                                               float2 *__restrict__ plane, uint32_t stride, BinHeader *__restrict__ reset) {
    if (reset != nullptr && blockIdx.x == 0 && threadIdx.x == 0) reset->gmax_bits = 0;
    const uint32_t m = blockIdx.x * 256 + threadIdx.x;
    if (m >= stride) return;                // stride is a multiple of 32: lane pairs (and DPP quads) are in or out together
    encode_tile_level(F32Rows{reinterpret_cast<const float2 *>(S)}, cell, threadIdx.x & 1u, unit_point(xyzs, min(m, M - 1), bound), plane + m);
}

// The codebook level of M points under K messages at once (hg_encode_codebook_planes_multi): S is K pre-sums row-interleaved, S[row][k] (float2), so one corner
// of one point is ONE contiguous read of 8 K bytes for all messages.  A group of G consecutive lanes shares a point: lane j of the group reads, of each of the
// point's eight rows, messages 2 j and 2 j + 1 as one 16-byte load (kPair: K even, G = K / 2) or message j as one 8-byte load (K odd, G = K) -- a group's loads
// of a row are adjacent, a wave's instruction touches 64 / G rows instead of 64.  Every lane derives its point's rows and weights itself (corner_rows; no lane
// exchange, so groups may straddle waves), interpolates with trilerp as encode_tile_level does -- plane k has the bits of hg_encode_codebook_plane from S_k -- and
// writes cplanes[k][point].  Rows in [M, stride) replicate the last point, as there.
template <bool kPair>
__global__ void __launch_bounds__(256) k_encode_codebook_planes_multi(const float *__restrict__ xyzs, uint32_t M, float bound, float cell, const float2 *__restrict__ S,
                                                                      uint32_t K, uint32_t G, float2 *__restrict__ cplanes, uint32_t stride) {
    const uint64_t gid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t m = (uint32_t)(gid / G), j = (uint32_t)(gid - (uint64_t)m * G);
    if (m >= stride) return;
    const float3 p = unit_point(xyzs, min(m, M - 1), bound);
    Corner8 c;
    corner_rows(p.x, p.y, p.z, cell, c);
    float2 e[8];
    if constexpr (kPair) {
        float4 v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = *reinterpret_cast<const float4 *>(S + (size_t)c.row[q] * K + 2 * j);
#pragma unroll
        for (int q = 0; q < 8; ++q) e[q] = make_float2(v[q].x, v[q].y);
        cplanes[(size_t)(2 * j) * stride + m] = trilerp(e, c.wx, c.wy, c.wz);
#pragma unroll
        for (int q = 0; q < 8; ++q) e[q] = make_float2(v[q].z, v[q].w);
        cplanes[(size_t)(2 * j + 1) * stride + m] = trilerp(e, c.wx, c.wy, c.wz);
    } else {
#pragma unroll
        for (int q = 0; q < 8; ++q) e[q] = S[(size_t)c.row[q] * K + j];
        cplanes[(size_t)j * stride + m] = trilerp(e, c.wx, c.wy, c.wz);
    }
}

}  // namespace nsig

using namespace nsig;

// Level -> XCD-slot assignment of k_encode_planes: the six finest levels each get a slot of their own or share it only with coarse
// (cache-resident) levels; whole levels per slot.  The assignment that won round 1's same-box sweeps (profiles/r01_k_encoder_slots_sweep.txt); a
// cost-balanced split with levels cut across slots was measured slower (287-292 against 283 us, profiles/r02_encoder_experiments.txt: with all eight
// XCDs busy the launch is bound chip-wide by L2->L1 line fills, not by its fullest slot) and is gone.
static SlotTable default_slots(bool with_codebook) {
    static const uint8_t kWith[8][4] = {{16, 255, 255, 255}, {15, 255, 255, 255}, {14, 0, 255, 255}, {13, 1, 255, 255}, {12, 2, 3, 255}, {11, 4, 5, 255}, {10, 9, 255, 255}, {8, 7, 6, 255}};
    static const uint8_t kWithout[8][4] = {{15, 255, 255, 255}, {14, 255, 255, 255}, {13, 255, 255, 255}, {12, 255, 255, 255}, {11, 0, 1, 255}, {10, 2, 3, 255}, {9, 8, 4, 255}, {7, 6, 5, 255}};
    SlotTable t{};
    for (int slot = 0; slot < 8; ++slot)
        for (int k = 0; k < 4; ++k) {
            const uint8_t l = (with_codebook ? kWith : kWithout)[slot][k];
            if (l != 255) t.level[slot][t.n[slot]++] = l;
        }
    return t;
}

NSIG_EXPORT int hg_warm_tables(const float *const *base_tables_host, const float *S, float *sink, nsig_stream_t stream) {
    NSIG_REQUIRE(sink != nullptr, "hg_warm_tables: sink is one writable float (never written)");
    TablePtrs base{};
    if (int e = fill_base_tables(base_tables_host, base, "hg_warm_tables")) return e;
    k_warm_tables<<<8 * 128, 256, 0, as_stream(stream)>>>(base, S, default_slots(S != nullptr), sink);
    return check_launch("hg_warm_tables");
}

NSIG_EXPORT size_t hg_planes_bytes(uint32_t M) { return (size_t)(NSIG_BASE_LEVELS + 1) * plane_stride(M) * sizeof(float2); }

// The launch of every hg_encode_planes* entry point, over fp32 or packed tables.
template <typename Tables>
static int launch_encode_planes(const char *who, const float *xyzs, uint32_t M, const uint32_t *rows_dev, float bound, const Tables &tables, void *planes, bool mixed,
                                nsig_stream_t stream) {
    NSIG_REQUIRE(xyzs && planes, "%s: null pointer", who);
    NSIG_REQUIRE(bound > 0.0f, "%s: bound must be positive", who);
    NSIG_REQUIRE(aligned8(planes), "%s: planes must be 8-byte aligned", who);
    if (M == 0) return NSIG_OK;
    const uint32_t stride = plane_stride(M);
    const bool with_codebook = tables.has_codebook();
    const SlotTable tab = default_slots(with_codebook);
    int covered[NSIG_BASE_LEVELS + 1] = {};     // slots that encode the level: exactly one
    for (int s = 0; s < 8; ++s)
        for (int i = 0; i < tab.n[s]; ++i) covered[tab.level[s][i]] += 1;
    for (int l = 0; l < NSIG_BASE_LEVELS + (with_codebook ? 1 : 0); ++l) NSIG_REQUIRE(covered[l] == 1, "%s: level %d is assigned to %d slots", who, l, covered[l]);
    NSIG_REQUIRE(with_codebook || covered[NSIG_BASE_LEVELS] == 0, "%s: slot table names the codebook level but there is no codebook table", who);
    const uint32_t tiles = ceil_div(stride, 256u);
    // tiles per XCD slot handled by distinct workgroups before they start looping: with one tile per workgroup (cap >= tiles) the block
    // render's launch takes 244-247 us against 258-261 us with 1024 looping workgroups per slot (same-box sweep, profiles/r01_k_encoder_grid_sweep.txt)
    const uint32_t per_slot = tiles < 8192u ? tiles : 8192u;
    with_flag(mixed, [&](auto kMixed) {
        k_encode_planes<Tables, decltype(kMixed)::value><<<per_slot * 8, 256, 0, as_stream(stream)>>>(xyzs, M, bound, tables, make_level_geom(), reinterpret_cast<float2 *>(planes), stride, tab, rows_dev);
    });
    return check_launch(who);
}

static int encode_planes_f32(const float *xyzs, uint32_t M, const uint32_t *rows_dev, float bound, const float *const *base_tables_host, const float *S, void *planes,
                             bool mixed, nsig_stream_t stream) {
    if (M == 0) return NSIG_OK;
    F32Tables tables{};
    tables.S = S;
    if (int e = fill_base_tables(base_tables_host, tables.base, "hg_encode_planes")) return e;
    return launch_encode_planes("hg_encode_planes", xyzs, M, rows_dev, bound, tables, planes, mixed, stream);
}

NSIG_EXPORT int hg_encode_planes(const float *xyzs, uint32_t M, float bound, const float *const *base_tables_host, const float *S, void *planes,
                                 nsig_stream_t stream) {
    return encode_planes_f32(xyzs, M, nullptr, bound, base_tables_host, S, planes, false, stream);
}

NSIG_EXPORT int hg_encode_planes_rows(const float *xyzs, uint32_t M_capacity, const uint32_t *rows_dev, float bound, const float *const *base_tables_host,
                                      const float *S, void *planes, nsig_stream_t stream) {
    NSIG_REQUIRE(rows_dev != nullptr, "hg_encode_planes_rows: null row count");
    return encode_planes_f32(xyzs, M_capacity, rows_dev, bound, base_tables_host, S, planes, false, stream);
}

NSIG_EXPORT int hg_encode_planes_mixed(const float *xyzs, uint32_t M_capacity, const uint32_t *rows_dev, float bound, const float *const *base_tables_host,
                                       const float *S, void *planes, nsig_stream_t stream) {
    NSIG_REQUIRE(mlp_get_precision() == 1, "hg_encode_planes_mixed: the mixed layout carries the fp16 MLP's operands (mlp_set_precision(1))");
    return encode_planes_f32(xyzs, M_capacity, rows_dev, bound, base_tables_host, S, planes, true, stream);
}

template <int FMT>
static int encode_planes_packed(const float *xyzs, uint32_t M, const uint32_t *rows_dev, float bound, const void *const *tables_host, const float *params, void *planes,
                                bool mixed, nsig_stream_t stream) {
    const char *who = "hg_encode_planes_packed";
    PackedTables<FMT> tables{};
    tables.params = reinterpret_cast<const float2 *>(params);
    for (uint32_t i = 0; i <= NSIG_BASE_LEVELS; ++i) {
        NSIG_REQUIRE((tables_host[i] != nullptr || i == NSIG_BASE_LEVELS) && aligned16(tables_host[i]), "%s: table %u is null or not 16-byte aligned", who, i);
        tables.p[i] = tables_host[i];
    }
    return launch_encode_planes(who, xyzs, M, rows_dev, bound, tables, planes, mixed, stream);
}

// hg_encode_planes[_rows|_mixed] over packed tables.
NSIG_EXPORT int hg_encode_planes_packed(const float *xyzs, uint32_t M_capacity, const uint32_t *rows_dev, float bound, const void *const *tables_host, int format,
                                        const float *params, void *planes, int planes_layout, nsig_stream_t stream) {
    NSIG_REQUIRE(pk_row_bytes(format) != 0, "hg_encode_planes_packed: unknown format %d (0 f16, 1 q8, 2 q4)", format);
    if (int e = check_layout(planes_layout, "hg_encode_planes_packed")) return e;
    const bool mixed = planes_layout == NSIG_PLANES_MIXED;
    NSIG_REQUIRE(!mixed || mlp_get_precision() == 1, "hg_encode_planes_packed: the mixed layout carries the fp16 MLP's operands (mlp_set_precision(1))");
    NSIG_REQUIRE(tables_host, "hg_encode_planes_packed: null pointer");
    NSIG_REQUIRE(format == NSIG_PACK_F16 || params != nullptr, "hg_encode_planes_packed: the q8 and q4 formats need the per-table parameters (params, pk_pack_tables')");
    NSIG_REQUIRE(aligned8(planes) && aligned8(params), "hg_encode_planes_packed: planes and params must be 8-byte aligned");
    if (format == NSIG_PACK_F16) return encode_planes_packed<NSIG_PACK_F16>(xyzs, M_capacity, rows_dev, bound, tables_host, params, planes, mixed, stream);
    if (format == NSIG_PACK_Q8) return encode_planes_packed<NSIG_PACK_Q8>(xyzs, M_capacity, rows_dev, bound, tables_host, params, planes, mixed, stream);
    return encode_planes_packed<NSIG_PACK_Q4>(xyzs, M_capacity, rows_dev, bound, tables_host, params, planes, mixed, stream);
}

NSIG_EXPORT int hg_encode_codebook_plane(const float *xyzs, uint32_t M, float bound, const float *S, void *planes, int planes_layout, void *plan_to_reset,
                                         nsig_stream_t stream) {
    if (M == 0) return NSIG_OK;
    if (int e = check_layout(planes_layout, "hg_encode_codebook_plane")) return e;
    NSIG_REQUIRE(xyzs && S && planes, "hg_encode_codebook_plane: null pointer");
    NSIG_REQUIRE(bound > 0.0f, "hg_encode_codebook_plane: bound must be positive");
    NSIG_REQUIRE(aligned8(planes), "hg_encode_codebook_plane: planes must be 8-byte aligned");
    NSIG_REQUIRE(plan_to_reset == nullptr || aligned16(plan_to_reset), "hg_encode_codebook_plane: plan must be 16-byte aligned");
    const uint32_t stride = plane_stride(M);
    k_encode_codebook_plane<<<ceil_div(stride, 256u), 256, 0, as_stream(stream)>>>(xyzs, M, bound, make_level_geom().cell[NSIG_BASE_LEVELS], S,
                                                                                  plane_dest(planes, stride, planes_layout == NSIG_PLANES_MIXED, NSIG_BASE_LEVELS, 0), stride,
                                                                                  reinterpret_cast<BinHeader *>(plan_to_reset));
    return check_launch("hg_encode_codebook_plane");
}

// ---- K messages over one set of points (hg_codebook_presum_multi in hashgrid.hip makes S_multi)
NSIG_EXPORT size_t hg_multi_planes_bytes(uint32_t M, uint32_t K) { return (size_t)K * plane_stride(M) * sizeof(float2); }

NSIG_EXPORT int hg_encode_codebook_planes_multi(const float *xyzs, uint32_t M, float bound, const void *S_multi, uint32_t K, void *cplanes, nsig_stream_t stream) {
    NSIG_REQUIRE(xyzs && S_multi && cplanes, "hg_encode_codebook_planes_multi: null pointer");
    if (int e = check_multi_k(K, "hg_encode_codebook_planes_multi")) return e;
    NSIG_REQUIRE(bound > 0.0f, "hg_encode_codebook_planes_multi: bound must be positive");
    NSIG_REQUIRE(aligned16(S_multi), "hg_encode_codebook_planes_multi: S_multi must be 16-byte aligned");
    NSIG_REQUIRE(aligned8(cplanes), "hg_encode_codebook_planes_multi: cplanes must be 8-byte aligned");
    NSIG_REQUIRE(M <= (1u << 27), "hg_encode_codebook_planes_multi: M=%u too large", M);
    if (M == 0) return NSIG_OK;
    const uint32_t stride = plane_stride(M);
    const bool pair = (K & 1u) == 0u;
    const uint32_t G = pair ? K / 2 : K;
    const uint32_t grid = (uint32_t)(((uint64_t)stride * G + 255) / 256);
    const float cell = make_level_geom().cell[NSIG_BASE_LEVELS];
    const float2 *S = reinterpret_cast<const float2 *>(S_multi);
    with_flag(pair, [&](auto kPair) {
        k_encode_codebook_planes_multi<decltype(kPair)::value><<<grid, 256, 0, as_stream(stream)>>>(xyzs, M, bound, cell, S, K, G, reinterpret_cast<float2 *>(cplanes), stride);
    });
    return check_launch("hg_encode_codebook_planes_multi");
}
