/*
 * kmp_sweep_dev.h -- what the kernels that decide a payload from its bytes behind the marking pass share (kmp_relations.hip,
 * kmp_chains.hip): the payload's text end and "does this pattern start at this offset".  Device code only; a match is what the marking
 * pass marks (see the top of kmp_relations.hip).
 */
#ifndef KMP_SWEEP_DEV_H
#define KMP_SWEEP_DEV_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kmp_device.h"

namespace {

__device__ __forceinline__ uint32_t zero_bytes(uint32_t w) { return (w - 0x01010101u) & ~w & 0x80808080u; }

/* index of the first 0x00 among the 16 bytes of v, 16 where there is none (the lowest flagged byte of zero_bytes is exact) */
__device__ __forceinline__ uint32_t first_nul16(uint4 v)
{
    const uint32_t z0 = zero_bytes(v.x), z1 = zero_bytes(v.y), z2 = zero_bytes(v.z), z3 = zero_bytes(v.w);
    if (z0) return (uint32_t)__builtin_ctz(z0) >> 3;
    if (z1) return 4u + ((uint32_t)__builtin_ctz(z1) >> 3);
    if (z2) return 8u + ((uint32_t)__builtin_ctz(z2) >> 3);
    if (z3) return 12u + ((uint32_t)__builtin_ctz(z3) >> 3);
    return 16u;
}

/* E_k under the reference's rule: min(len, index of the payload's first 0x00).  Wave-uniform. */
__device__ __forceinline__ uint32_t text_end(const uint8_t *__restrict__ payload, uint32_t len, uint32_t lane)
{
    for (uint32_t base = 0; base < len; base += KMP_CHUNK) {
        const uint32_t p = base + lane * KMP_LANE_BYTES;
        uint32_t z = 16u;
        if (p < len) z = first_nul16(*reinterpret_cast<const uint4 *>(payload + p));
        const bool found = z < 16u && p + z < len;
        const uint64_t b = __ballot(found);
        if (b != 0ull) return (uint32_t)__builtin_amdgcn_readlane((int)(p + z), (int)__builtin_ctzll(b));
    }
    return len;
}

/* Does pattern `pat` of m bytes start at offset s of the text [0, E) at `text`, inside the window?  s differs from lane to lane, the
 * rest is wave-uniform.  A lane that is out (no such start, or a byte differed) loads nothing more. */
__device__ __forceinline__ bool match_at(const uint8_t *__restrict__ text, const uint8_t *__restrict__ pat, uint32_t m, long long s,
                                         long long E, uint2 win)
{
    bool ok = s >= 0 && s + (long long)m <= E && s >= (long long)win.x && s <= (long long)win.y;
    for (uint32_t i = 0; i < m && __ballot(ok) != 0ull; ++i) {
        uint8_t c = 0;
        if (ok) c = text[s + i];
        ok = ok && c == pat[i];
    }
    return ok;
}

}  // namespace

#endif
