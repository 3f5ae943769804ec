// Packed tables of a released model (include/nerfsig.h "packed released model"): the 17 fp32 tables of release.ReleasedModel stored as fp16
// pairs, 8-bit or 4-bit codes, with the quantiser of the tamper kernels (csrc/tamper.hip: NSIG_TAMPER_HALF, NSIG_TAMPER_QUANTIZE at 8 / 4 bits) -- so that
// decode(pack(x)) is, bit for bit, what tm_apply leaves in the fp32 table.  The encoder that gathers from such tables is in csrc/encode.hip
// (k_encode_planes<PackedTables<FMT>, mixed>); the row words and their decode in csrc/packed.h.
//
//   pack    one launch over the whole list: workgroup (table, chunk) turns 1024 rows (8 KiB of fp32) into 4 KiB / 2 KiB / 1 KiB of row words; a thread reads its four
//           rows as two 16-byte loads and writes them as ONE 16-, 8- or 4-byte store.  lo and step are computed by every workgroup from the table's statistics
//           (TmScalars' arithmetic); chunk 0 also stores them to params.  Non-finite values (q formats) are counted per wave and added to the device word with one
//           integer atomic per wave that found any -- the sum does not depend on the order.
//   unpack  the reverse walk: one 16-, 8- or 4-byte load, two 16-byte stores.
// No host read, no allocation; the word is cleared by a stream-ordered memset in front of the launch.  Compiled with -ffp-contract=off like the rest.
#include <math.h>

#include "packed.h"

namespace nsig {

constexpr uint32_t kPkTables = NSIG_BASE_LEVELS + 1;       // at most 17 tables per call
constexpr uint32_t kPkThreads = 256, kPkRowsPerThread = 4, kPkChunkRows = kPkThreads * kPkRowsPerThread;
constexpr uint32_t kPkChunks = NSIG_TABLE_ROWS / kPkChunkRows;      // 512 workgroups per table
static_assert(NSIG_TABLE_ROWS % kPkChunkRows == 0, "a table is a whole number of chunks");

struct PkList {
    const void *src[kPkTables];
    void *dst[kPkTables];
};

__device__ inline bool pk_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// q = min(L, max(0, rintf((x - lo) / step))) as NSIG_TAMPER_QUANTIZE computes it; a constant table (pass) and a non-finite value take code 0
__device__ __forceinline__ uint32_t pk_code(float x, float lo, float step, float L, bool pass, uint32_t &bad) {
    if (!pk_finite(x)) {
        bad += 1u;
        return 0u;
    }
    if (pass) return 0u;
    return (uint32_t)fminf(L, fmaxf(0.0f, rintf((x - lo) / step)));
}

template <int FMT>
__global__ void __launch_bounds__(kPkThreads) k_pk_pack(PkList a, const double *__restrict__ stats, float2 *__restrict__ params, uint32_t *__restrict__ nonfinite) {
    const uint32_t t = blockIdx.x / kPkChunks, chunk = blockIdx.x % kPkChunks;
    const uint32_t row = chunk * kPkChunkRows + kPkRowsPerThread * threadIdx.x;      // < NSIG_TABLE_ROWS: the grid is n * kPkChunks
    const float4 *x = reinterpret_cast<const float4 *>(reinterpret_cast<const float *>(a.src[t]) + 2 * (size_t)row);
    const float4 v0 = x[0], v1 = x[1];      // rows (row, row + 1), (row + 2, row + 3)
    if (FMT == NSIG_PACK_F16) {
        uint4 w;
        w.x = pk_half_pair(v0.x, v0.y); w.y = pk_half_pair(v0.z, v0.w); w.z = pk_half_pair(v1.x, v1.y); w.w = pk_half_pair(v1.z, v1.w);
        reinterpret_cast<uint4 *>(a.dst[t])[row / 4] = w;
        return;
    }
    constexpr uint32_t bits = FMT == NSIG_PACK_Q8 ? 8u : 4u;
    const float L = (float)((1u << bits) - 1u);
    const float lo = (float)stats[(size_t)t * 4], hi = (float)stats[(size_t)t * 4 + 1];      // TmScalars (csrc/tamper.hip)
    const float step = (hi - lo) / L;
    const bool pass = hi == lo;
    if (chunk == 0 && threadIdx.x == 0) params[t] = make_float2(lo, step);      // (a constant table: step = 0, every code 0, decode = lo)
    uint32_t bad = 0u;
    const float f[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
    uint32_t q[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) q[k] = pk_code(f[k], lo, step, L, pass, bad);
    if (FMT == NSIG_PACK_Q8) {
        uint2 w;
        w.x = q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24);
        w.y = q[4] | (q[5] << 8) | (q[6] << 16) | (q[7] << 24);
        reinterpret_cast<uint2 *>(a.dst[t])[row / 4] = w;
    } else {
        uint32_t w = 0u;
#pragma unroll
        for (int k = 0; k < 8; ++k) w |= q[k] << (4 * k);
        reinterpret_cast<uint32_t *>(a.dst[t])[row / 4] = w;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) bad += __shfl_xor(bad, d, 64);
    if ((threadIdx.x & 63u) == 0u && bad != 0u) atomicAdd(nonfinite, bad);
}

template <int FMT>
__global__ void __launch_bounds__(kPkThreads) k_pk_unpack(PkList a, const float2 *__restrict__ params) {
    const uint32_t t = blockIdx.x / kPkChunks, chunk = blockIdx.x % kPkChunks;
    const uint32_t row = chunk * kPkChunkRows + kPkRowsPerThread * threadIdx.x;
    float2 ps = make_float2(0.0f, 0.0f);
    if (FMT != NSIG_PACK_F16) ps = params[t];
    uint32_t w[4];
    if (FMT == NSIG_PACK_F16) {
        const uint4 v = reinterpret_cast<const uint4 *>(a.src[t])[row / 4];
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    } else if (FMT == NSIG_PACK_Q8) {
        const uint2 v = reinterpret_cast<const uint2 *>(a.src[t])[row / 4];
        w[0] = v.x & 0xffffu; w[1] = v.x >> 16; w[2] = v.y & 0xffffu; w[3] = v.y >> 16;
    } else {
        const uint32_t v = reinterpret_cast<const uint32_t *>(a.src[t])[row / 4];
        w[0] = v & 0xffu; w[1] = (v >> 8) & 0xffu; w[2] = (v >> 16) & 0xffu; w[3] = v >> 24;
    }
    const float2 r0 = pk_decode_row<FMT>(w[0], ps.x, ps.y), r1 = pk_decode_row<FMT>(w[1], ps.x, ps.y);
    const float2 r2 = pk_decode_row<FMT>(w[2], ps.x, ps.y), r3 = pk_decode_row<FMT>(w[3], ps.x, ps.y);
    float4 *y = reinterpret_cast<float4 *>(reinterpret_cast<float *>(a.dst[t]) + 2 * (size_t)row);
    y[0] = make_float4(r0.x, r0.y, r1.x, r1.y);
    y[1] = make_float4(r2.x, r2.y, r3.x, r3.y);
}

static int pk_check(const char *who, const void *const *src_host, uint32_t n, int format, void *const *dst_host, PkList &a) {
    NSIG_REQUIRE(pk_row_bytes(format) != 0, "%s: unknown format %d (0 f16, 1 q8, 2 q4)", who, format);
    NSIG_REQUIRE(src_host && dst_host, "%s: null pointer", who);
    NSIG_REQUIRE(n >= 1 && n <= kPkTables, "%s: n = %u tables is out of range (1 .. %u)", who, n, kPkTables);
    for (uint32_t i = 0; i < n; ++i) {
        NSIG_REQUIRE(src_host[i] && dst_host[i] && aligned16(src_host[i]) && aligned16(dst_host[i]), "%s: table %u is null or not 16-byte aligned", who, i);
        a.src[i] = src_host[i];
        a.dst[i] = dst_host[i];
    }
    return NSIG_OK;
}

}  // namespace nsig

using namespace nsig;

NSIG_EXPORT size_t pk_table_bytes(int format) { return (size_t)NSIG_TABLE_ROWS * pk_row_bytes(format); }

NSIG_EXPORT int pk_pack_tables(const float *const *src_host, uint32_t n, int format, const double *stats, void *const *dst_host, float *params, uint32_t *nonfinite,
                               nsig_stream_t stream) {
    PkList a{};
    if (int e = pk_check("pk_pack_tables", reinterpret_cast<const void *const *>(src_host), n, format, dst_host, a)) return e;
    NSIG_REQUIRE(format == NSIG_PACK_F16 || (stats && params && nonfinite), "pk_pack_tables: the q8 and q4 formats need stats (tm_stats'), params and nonfinite");
    NSIG_REQUIRE(aligned8(stats) && aligned8(params) && aligned4(nonfinite), "pk_pack_tables: stats and params must be 8-byte aligned, nonfinite 4-byte aligned");
    hipStream_t st = as_stream(stream);
    if (nonfinite != nullptr && hipMemsetAsync(nonfinite, 0, sizeof(uint32_t), st) != hipSuccess) {
        set_error("pk_pack_tables: cannot clear the non-finite word");
        return NSIG_ERR_LAUNCH;
    }
    float2 *ps = reinterpret_cast<float2 *>(params);
    if (format == NSIG_PACK_F16) k_pk_pack<NSIG_PACK_F16><<<n * kPkChunks, kPkThreads, 0, st>>>(a, stats, ps, nonfinite);
    else if (format == NSIG_PACK_Q8) k_pk_pack<NSIG_PACK_Q8><<<n * kPkChunks, kPkThreads, 0, st>>>(a, stats, ps, nonfinite);
    else k_pk_pack<NSIG_PACK_Q4><<<n * kPkChunks, kPkThreads, 0, st>>>(a, stats, ps, nonfinite);
    return check_launch("pk_pack_tables");
}

NSIG_EXPORT int pk_unpack_tables(const void *const *src_host, uint32_t n, int format, const float *params, float *const *dst_host, nsig_stream_t stream) {
    PkList a{};
    if (int e = pk_check("pk_unpack_tables", src_host, n, format, reinterpret_cast<void *const *>(dst_host), a)) return e;
    NSIG_REQUIRE(format == NSIG_PACK_F16 || params != nullptr, "pk_unpack_tables: the q8 and q4 formats need the per-table parameters (params, pk_pack_tables')");
    NSIG_REQUIRE(aligned8(params), "pk_unpack_tables: params must be 8-byte aligned");
    hipStream_t st = as_stream(stream);
    const float2 *ps = reinterpret_cast<const float2 *>(params);
    if (format == NSIG_PACK_F16) k_pk_unpack<NSIG_PACK_F16><<<n * kPkChunks, kPkThreads, 0, st>>>(a, ps);
    else if (format == NSIG_PACK_Q8) k_pk_unpack<NSIG_PACK_Q8><<<n * kPkChunks, kPkThreads, 0, st>>>(a, ps);
    else k_pk_unpack<NSIG_PACK_Q4><<<n * kPkChunks, kPkThreads, 0, st>>>(a, ps);
    return check_launch("pk_unpack_tables");
}
