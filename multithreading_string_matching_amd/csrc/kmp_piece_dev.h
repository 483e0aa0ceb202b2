/*
 * kmp_piece_dev.h -- device helpers of the gathers that build a derived arena from byte ranges of a source arena (kmp_seams.hip, kmp_streams.hip, kmp_streams_seq.hip,
 * kmp_fields.hip): the 16 bytes of a range that starts at any byte, from aligned 16-byte units.  gfx950.
 */
#ifndef KMP_PIECE_DEV_H
#define KMP_PIECE_DEV_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kmp_unit_dev.h"

namespace kmp_piece {

using kmp_unit::u32x4;          /* the unit, its loads and stores and the one byte mask: kmp_unit_dev.h */
using kmp_unit::load_unit;
using kmp_unit::store_unit;
using kmp_unit::below_mask;

/* The 16 bytes [start, start + 16) of a piece, in coordinates relative to `base` (16-byte aligned), of which [lo, hi) exist (0 <= lo <= hi);
 * start >= -15.  Bytes outside [lo, hi) come out 0x00.  Only the aligned units that hold a byte of [lo, hi) are loaded. */
template <bool NT>
__device__ __forceinline__ u32x4 fetch_piece(const uint8_t *base, int32_t start, int32_t lo, int32_t hi)
{
    const int32_t a0 = start & ~15;                                  /* (arithmetic: -16 for a negative start) */
    const uint32_t s = (uint32_t)(start - a0);
    const int32_t klo = min(max(lo - start, 0), 16), khi = min(max(hi - start, 0), 16);
    u32x4 r = (u32x4)(0u);
    if (klo >= khi) return r;
    /* the bytes wanted are [start + klo, start + khi): the first unit holds some where start + klo < a0 + 16, the second where
     * start + khi > a0 + 16; a0 < 0 is never wanted (lo >= 0) */
    u32x4 u0 = (u32x4)(0u), u1 = (u32x4)(0u);
    if (start + klo < a0 + 16) u0 = load_unit<NT>(base + a0);
    if (start + khi > a0 + 16) u1 = load_unit<NT>(base + a0 + 16);
    uint32_t w[9] = {u0.x, u0.y, u0.z, u0.w, u1.x, u1.y, u1.z, u1.w, 0u};
    /* by whole dwords, then by bytes */
    if (s & 8u) {
#pragma unroll
        for (uint32_t i = 0; i < 7u; ++i) w[i] = w[i + 2u];
    }
    if (s & 4u) {
#pragma unroll
        for (uint32_t i = 0; i < 6u; ++i) w[i] = w[i + 1u];
    }
    uint32_t o[4];
#pragma unroll
    for (uint32_t d = 0; d < 4u; ++d)
        o[d] = __builtin_amdgcn_alignbyte(w[d + 1u], w[d], s & 3u) & below_mask((uint32_t)khi, d) & ~below_mask((uint32_t)klo, d);
    r.x = o[0]; r.y = o[1]; r.z = o[2]; r.w = o[3];
    return r;
}

}  // namespace kmp_piece

#endif
