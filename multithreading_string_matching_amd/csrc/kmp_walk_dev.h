/*
 * kmp_walk_dev.h -- device helpers of the locates that walk a length-prefixed structure forward through a payload, a lane per payload
 * (kmp_dns.hip, kmp_tls.hip): one aligned 16-byte unit of the payload is held in registers, a byte comes out of it by selects and a
 * shift, and the next unit is loaded when the walk leaves the held one; and of their gathers, which put a separator over the length
 * bytes from a bit mask.  gfx950.
 */
#ifndef KMP_WALK_DEV_H
#define KMP_WALK_DEV_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kmp_unit_dev.h"

namespace kmp_walk {

using kmp_unit::u32x4;
using kmp_unit::load_unit;

/* byte q (0 .. 15) of a unit: two selects and a shift, no register indexing */
__device__ __forceinline__ uint32_t unit_byte(u32x4 v, uint32_t q)
{
    const uint32_t lo = (q & 4u) ? v.y : v.x, hi = (q & 4u) ? v.w : v.z;
    return (((q & 8u) ? hi : lo) >> (8u * (q & 3u))) & 0xFFu;
}

/* the byte at `pos` of the payload at p; `held` is the aligned unit `hu` of it.  pos lies in front of the payload's end. */
__device__ __forceinline__ uint32_t walk_byte(const uint8_t *p, uint32_t pos, u32x4 &held, uint32_t &hu)
{
    if ((pos >> 4) != hu) {
        hu = pos >> 4;
        held = load_unit<false>(p + 16ull * hu);
    }
    return unit_byte(held, pos & 15u);
}

/* for the gathers that put a separator over the length bytes: 0xFF in every byte of a dword whose bit of the nibble is set */
__device__ __forceinline__ uint32_t spread4(uint32_t nib) { return (((nib & 15u) * 0x00204081u) & 0x01010101u) * 0xFFu; }

}  // namespace kmp_walk

#endif
