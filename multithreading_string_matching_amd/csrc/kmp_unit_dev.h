/*
 * kmp_unit_dev.h -- the 16-byte unit every arena builder moves payload bytes in, and what the builders share around it: its loads and
 * stores, the one byte mask (below_mask, keep_bytes), byte classes by SWAR compares on dwords, the wavefront's scans, the sync of a wavefront's own
 * LDS, and the units of a RUN of consecutive payloads dealt to the lanes in order (Unit, find_payload, load_step).  The skeleton built
 * on these is kmp_compact_dev.h.  Device code only; gfx950.
 */
#ifndef KMP_UNIT_DEV_H
#define KMP_UNIT_DEV_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kmp_device.h"

namespace kmp_unit {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

/* ---- byte classes of a dword, 0x80 in every byte of the class, and those four bits gathered into bits 0..3 ---- */
static __device__ __forceinline__ uint32_t eq_bytes(uint32_t w, uint32_t c4)
{
    const uint32_t x = w ^ c4;
    return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
}
static __device__ __forceinline__ uint32_t bits4(uint32_t t) { return ((t >> 7) * 0x10204080u) >> 28; }
static __device__ __forceinline__ uint32_t eq16(u32x4 v, uint32_t c4)
{
    return bits4(eq_bytes(v.x, c4)) | bits4(eq_bytes(v.y, c4)) << 4 | bits4(eq_bytes(v.z, c4)) << 8 | bits4(eq_bytes(v.w, c4)) << 12;
}

/* the positions of a unit that lie inside a payload of which `left` bytes remain at the unit's start */
static __device__ __forceinline__ uint32_t valid_bits(uint32_t left) { return left >= 16u ? 0xFFFFu : (1u << left) - 1u; }

/* Inclusive sum over the wavefront (all 64 lanes active): four shifts inside the rows of 16, then the rows' totals handed on. */
static __device__ __forceinline__ uint32_t wave_incl_scan(uint32_t x)
{
    int v = (int)x;
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, false);          /* row_shr:1 */
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, false);          /* row_shr:2 */
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, false);          /* row_shr:4 */
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, false);          /* row_shr:8 */
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, false);          /* row_bcast:15 into rows 1 and 3 */
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, false);          /* row_bcast:31 into rows 2 and 3 */
    return (uint32_t)v;
}
/* ... of 64-bit values, once per run: the unit counts of 64 payloads of up to 2^30 bytes do not fit 32 bits */
static __device__ __forceinline__ uint64_t wave_incl_scan64(uint64_t v, uint32_t lane)
{
#pragma unroll
    for (uint32_t d = 1; d < KMP_WAVE; d <<= 1) {
        const uint64_t t = __shfl_up((unsigned long long)v, d);
        if (lane >= d) v += t;
    }
    return v;
}
static __device__ __forceinline__ uint64_t bcast64(uint64_t v, uint32_t from) { return (uint64_t)__shfl((unsigned long long)v, (int)from); }

template <bool NT>
static __device__ __forceinline__ u32x4 load_unit(const uint8_t *p)
{
    const u32x4 *q = reinterpret_cast<const u32x4 *>(p);
    return NT ? __builtin_nontemporal_load(q) : *q;
}
template <bool NT>
static __device__ __forceinline__ void store_unit(uint8_t *p, u32x4 v)
{
    u32x4 *q = reinterpret_cast<u32x4 *>(p);
    if (NT) __builtin_nontemporal_store(v, q); else *q = v;
}

/* The one byte mask: 0xFF in the bytes below position x of dword d of a unit (byte positions 4 d .. 4 d + 3), 0 <= x; x >= 16: all */
static __device__ __forceinline__ uint32_t below_mask(uint32_t x, uint32_t d)
{
    const uint32_t b = 4u * d;
    return (x >= b + 4u) ? 0xFFFFFFFFu : (x <= b) ? 0u : ((1u << (8u * (x - b))) - 1u);
}
/* the bytes [keep, 16) of a unit cleared; keep >= 16 leaves it whole */
static __device__ __forceinline__ u32x4 keep_bytes(u32x4 v, uint32_t keep)
{
    u32x4 r;
    r.x = v.x & below_mask(keep, 0u); r.y = v.y & below_mask(keep, 1u); r.z = v.z & below_mask(keep, 2u); r.w = v.w & below_mask(keep, 3u);
    return r;
}

/* the wavefront's own LDS: its DS instructions execute in order, the barriers keep the compiler from moving them */
static __device__ __forceinline__ void lds_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

/* One unit of a step, as both kernels see it. */
struct Unit {
    u32x4 v;            /* the 16 bytes, 0 for a lane without a unit */
    uint32_t  p;            /* payload of the run */
    uint32_t  rel, len;     /* the unit's offset in its payload, the payload's length */
    uint32_t  first;        /* lane of this step that holds the payload's first unit, 0 where that unit lies in an earlier step */
    bool      act, started; /* the lane has a unit; its payload began in an earlier step */
};

/* The run's tables and the search.  s_ub: units of the run before payload i. */
static __device__ __forceinline__ uint32_t find_payload(const uint64_t *s_ub, uint64_t g)
{
    uint32_t p = 0u;                                            /* the last payload of the run that starts at or before unit g */
#pragma unroll
    for (uint32_t step = KMP_WAVE / 2u; step; step >>= 1)
        if (s_ub[p + step] <= g) p += step;
    return p;
}

template <bool NT>
static __device__ __forceinline__ void load_step(Unit &un, const uint8_t *src, const uint64_t *s_ub, const uint64_t *s_src, const uint32_t *s_len,
                                          uint64_t gs, uint64_t total_units, uint32_t lane)
{
    const uint64_t g = gs + lane;
    un.act = g < total_units;
    un.v = (u32x4)(0u);
    un.p = 0u; un.rel = 0u; un.len = 0u; un.first = 0u; un.started = false;
    if (un.act) {
        un.p = find_payload(s_ub, g);
        const uint64_t ub = s_ub[un.p];
        un.rel = (uint32_t)(g - ub) * 16u;
        un.len = s_len[un.p];
        un.started = ub < gs;
        un.first = un.started ? 0u : (uint32_t)(ub - gs);
        un.v = load_unit<NT>(src + s_src[un.p] + un.rel);
    }
}

}  // namespace kmp_unit

#endif
