// Row words of a PACKED table (include/nerfsig.h "packed released model"): what csrc/packed.hip writes and what the packed row source of csrc/encode.hip gathers.
// A table is NSIG_TABLE_ROWS rows of 2 features; a row is ONE word of 4 (f16), 2 (q8) or 1 (q4) bytes, feature 0 in its low half.
//   decode:  f16  (float)(_Float16)h
//            q8 / q4  lo + (float)q * step -- the product and the sum each rounded on its own (written with the explicit round-to-nearest intrinsics, and the
//            library is built with -ffp-contract=off): the float NSIG_TAMPER_QUANTIZE leaves in the fp32 table for the same code q.
#pragma once

#include "common.h"

namespace nsig {

__host__ __device__ inline uint32_t pk_row_bytes(int format) {
    return format == NSIG_PACK_F16 ? 4u : (format == NSIG_PACK_Q8 ? 2u : (format == NSIG_PACK_Q4 ? 1u : 0u));
}

// The row word of `row`, fetched as the ALIGNED 8 BYTES around it (one global_load_dwordx2) and cut out in registers.  A gather of 4-, 2- or 1-byte elements is
// served markedly slower than one of 8-byte elements touching the same lines (the encoder launch 272-274 us with narrow loads, 202-213 us
// with these, 230 us for the fp32 tables); the shifts hide under the address path.  A table is 16-byte aligned and a multiple of 8 bytes long: the 8 bytes lie inside it.
template <int FMT>
__device__ __forceinline__ uint32_t pk_load_row(const void *__restrict__ table, uint32_t row) {
    const uint32_t byte = row * (FMT == NSIG_PACK_F16 ? 4u : (FMT == NSIG_PACK_Q8 ? 2u : 1u));      // < pk_table_bytes(FMT): row < NSIG_TABLE_ROWS
    const uint2 w = *reinterpret_cast<const uint2 *>(reinterpret_cast<const char *>(table) + (byte & ~7u));
    const uint32_t d = (byte & 4u) ? w.y : w.x;
    if (FMT == NSIG_PACK_F16) return d;
    if (FMT == NSIG_PACK_Q8) return (d >> ((byte & 2u) * 8u)) & 0xffffu;
    return (d >> ((byte & 3u) * 8u)) & 0xffu;
}

// the f16 row word of (a, b): each through (_Float16), round to nearest even, above 65504 infinity -- NSIG_TAMPER_HALF's conversion
__device__ __forceinline__ uint32_t pk_half_pair(float a, float b) {
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    const h2 h = {(_Float16)a, (_Float16)b};
    return __builtin_bit_cast(uint32_t, h);
}

__device__ __forceinline__ float pk_dequant(uint32_t q, float lo, float step) { return __fadd_rn(lo, __fmul_rn((float)q, step)); }

template <int FMT>
__device__ __forceinline__ float2 pk_decode_row(uint32_t w, float lo, float step) {
    if (FMT == NSIG_PACK_F16) {
        typedef _Float16 h2 __attribute__((ext_vector_type(2)));
        const h2 h = __builtin_bit_cast(h2, w);
        return make_float2((float)h[0], (float)h[1]);
    }
    if (FMT == NSIG_PACK_Q8) return make_float2(pk_dequant(w & 0xffu, lo, step), pk_dequant((w >> 8) & 0xffu, lo, step));
    return make_float2(pk_dequant(w & 0xfu, lo, step), pk_dequant((w >> 4) & 0xfu, lo, step));
}

}  // namespace nsig
