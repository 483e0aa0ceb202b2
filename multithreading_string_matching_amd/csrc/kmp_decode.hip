/*
 * kmp_decode.hip -- kmpgpu_load_decoded: the payloads of an arena percent-decoded on the device into a packed arena (kmpgpu.h).  gfx950.
 *
 *   kmp_decode_lengths_kernel   dec_len[k] = decoded length of payload k, or 0xFFFFFFFF ("not in dst") for an unchanged payload under
 *                               KMPGPU_DECODE_ONLY_CHANGED; the changed bitmap, one plain store per word; bytes in / out and n_changed
 *   kmp_scan_local_kernel, kmp_scan_totals_kernel   of kmp_prep.hip, through kmp_launch_compact_scan
 *   kmp_decode_index_kernel     the new index, and per payload of dst the record {source offset, source length, decoded length}
 *   kmp_decode_write_kernel     the bytes
 *
 * The transform is decided position by position (kmpgpu.h): esc(i) = p[i] == '%' and p[i+1], p[i+2] hex digits inside the payload, a
 * position is consumed where esc(i-1) or esc(i-2).  Per 16-byte unit that is bit arithmetic on three 16-bit masks ('%', hex digit,
 * inside the payload) extended by the masks of the four bytes before and after the unit; a byte at or behind the payload's end has
 * no bit in any mask, so nothing behind it decodes, whatever the slot holds there.
 *
 * The four steps, the RUN of payloads whose 16-byte units are dealt to the lanes in order, the per-payload sums, the straight copy of a
 * step that changes nothing and the LDS stage of any other step are the compacting skeleton's (lengths_body, write_body:
 * kmp_compact_dev.h).  What is this file's own is the policy PercentDecode.  Consecutive lanes hold consecutive units, so the
 * neighbours' masks come through a lane shift; lane 0 takes the bytes before its unit from the step before, and lane 63 loads the unit
 * behind its own where its own ends in a '%'.  A step without a '%' in it or in the two bytes before it is known after one ballot
 * and emits every position.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kmp_device.h"
#include "kmp_launch.h"
#include "kmp_compact_dev.h"

namespace {

using namespace kmp_unit;     /* kmp_compact_dev.h: index_body, lengths_body, write_body; kmp_unit_dev.h: the unit, byte classes */

/* ---- byte classes of a dword, 0x80 in every byte of the class (eq_bytes, bits4, eq16: kmp_unit_dev.h) ---- */
__device__ __forceinline__ uint32_t hex_bytes(uint32_t w)
{
    const uint32_t lo7 = w & 0x7F7F7F7Fu;
    const uint32_t dig = (lo7 + 0x50505050u) & ~(lo7 + 0x46464646u);        /* 0x30 <= b <= 0x39 */
    const uint32_t l = lo7 | 0x20202020u;
    const uint32_t let = (l + 0x1F1F1F1Fu) & ~(l + 0x19191919u);            /* 0x61 <= b | 0x20 <= 0x66 */
    return (dig | let) & ~w & 0x80808080u;
}
__device__ __forceinline__ uint32_t hex16(u32x4 v)
{
    return bits4(hex_bytes(v.x)) | bits4(hex_bytes(v.y)) << 4 | bits4(hex_bytes(v.z)) << 8 | bits4(hex_bytes(v.w)) << 12;
}
constexpr uint32_t PCT4 = 0x25252525u, PLUS4 = 0x2B2B2B2Bu;

/* '%' and hex masks of a unit (bits 0..15, '%' | hex << 16), and what the four bytes on either side add (same packing: the unit
 * before, of which bits 12..15 count, and the one behind, of which bits 0..3 do) -> emitted positions and escape starts */
struct UnitMasks { uint32_t emit, esc; };
__device__ __forceinline__ UnitMasks unit_masks(uint32_t own, uint32_t prevm, uint32_t nextm, uint32_t valid)
{
    const uint32_t P = ((prevm >> 12) & 0xFu) | ((own & 0xFFFFu) << 4) | ((nextm & 0xFu) << 20);
    const uint32_t H = ((prevm >> 28) & 0xFu) | ((own >> 16) << 4) | (((nextm >> 16) & 0xFu) << 20);
    const uint32_t E = P & (H >> 1) & (H >> 2);                 /* esc(i), bit i + 4 */
    const uint32_t C = (E << 1) | (E << 2);                     /* consumed */
    UnitMasks m;
    m.esc = (E >> 4) & 0xFFFFu;
    m.emit = valid & ~(C >> 4) & 0xFFFFu;
    return m;
}

/* Masks of a unit with its neighbours' through the lane shift; lane 0 from hp, the last dword of the step before (its lane 63 held the
 * unit before), lane 63 from the unit behind its own, which it loads where its own ends in a '%'.  next_x: the four bytes
 * behind the unit where the payload has them (their values are needed where an escape starts at 14 or 15). */
__device__ __forceinline__ UnitMasks step_masks(const Unit &un, uint32_t hp, const uint8_t *addr, uint32_t lane, uint32_t valid, uint32_t P16,
                                                 uint32_t *next_x)
{
    const uint32_t own = P16 | (hex16(un.v) & valid) << 16;
    uint32_t prevm = __shfl_up(own, 1), nextm = __shfl_down(own, 1);
    uint32_t nx = __shfl_down(un.v.x, 1);
    if (lane == 0u) prevm = bits4(eq_bytes(hp, PCT4)) << 12 | bits4(hex_bytes(hp)) << 28;
    if (lane == KMP_WAVE - 1u) {
        nextm = 0u; nx = 0u;
        if (un.act && un.rel + 16u < un.len && (P16 & 0xC000u)) {
            /* the whole unit behind, as one load that is not narrowed: payload bytes move in 16-byte loads only */
            nx = (*(const volatile __attribute__((address_space(1))) u32x4 *)(uintptr_t)(addr + 16)).x;
            const uint32_t left = un.len - un.rel - 16u, vm = left >= 4u ? 0xFu : (1u << left) - 1u;
            nextm = (bits4(eq_bytes(nx, PCT4)) & vm) | (bits4(hex_bytes(nx)) & vm) << 16;
        }
    }
    if (un.rel == 0u) prevm = 0u;                               /* the lane before holds another payload's unit */
    if (un.rel + 16u >= un.len) nextm = 0u;                     /* ... and so does the lane behind */
    *next_x = nx;
    return unit_masks(own, prevm, nextm, valid);
}

__device__ __forceinline__ uint32_t hex_val(uint32_t c) { return (c & 0xFu) + (c >> 6) * 9u; }

/* The transform as lengths_body and write_body take it (kmp_compact_dev.h).  What a step hands on: the last four bytes of its last unit. */
struct PercentDecode {
    uint32_t plus;
    uint32_t tail_w;
    struct Step { uint32_t valid, emit, esc, plus16, next_x; bool changed; };

    __device__ __forceinline__ void reset() { tail_w = 0u; }
    __device__ __forceinline__ Step step(const Unit &q, const uint8_t *addr, uint32_t lane)
    {
        Step st;
        st.valid = q.act ? valid_bits(q.len - q.rel) : 0u;
        const uint32_t hp = (lane == 0u && q.rel) ? tail_w : 0u;
        tail_w = (uint32_t)__builtin_amdgcn_readlane((int)q.v.w, 63);
        const uint32_t P16 = eq16(q.v, PCT4) & st.valid;
        st.plus16 = plus ? eq16(q.v, PLUS4) & st.valid : 0u;
        st.emit = st.valid; st.esc = 0u; st.next_x = 0u;
        st.changed = st.plus16 != 0u;
        /* a step without a '%' in it, or in the two bytes before it, emits every position: most steps of most captures */
        if (__any(P16 | (bits4(eq_bytes(hp, PCT4)) & 0xCu))) {
            const UnitMasks m = step_masks(q, hp, addr, lane, st.valid, P16, &st.next_x);
            st.emit = m.emit; st.esc = m.esc;
            st.changed = st.changed || m.emit != st.valid || m.esc != 0u;       /* (an escape's own position is emitted, as another byte) */
        }
        return st;
    }
    __device__ __forceinline__ uint32_t byte(const Step &st, const Unit &q, uint32_t i) const
    {
        if (!((st.emit >> i) & 1u)) return 0u;
        const uint32_t w[5] = {q.v.x, q.v.y, q.v.z, q.v.w, st.next_x};
        if ((st.esc >> i) & 1u)
            return hex_val((w[(i + 1u) >> 2] >> (8u * ((i + 1u) & 3u))) & 0xFFu) << 4 | hex_val((w[(i + 2u) >> 2] >> (8u * ((i + 2u) & 3u))) & 0xFFu);
        if ((st.plus16 >> i) & 1u) return 0x20u;
        return (w[i >> 2] >> (8u * (i & 3u))) & 0xFFu;
    }
};

__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_decode_lengths_kernel(const uint8_t *__restrict__ src, const uint64_t *__restrict__ src_off, const uint32_t *__restrict__ src_len,
                          uint64_t n, uint32_t plus, uint32_t only_changed, uint32_t *__restrict__ dec_len,
                          unsigned long long *__restrict__ changed, unsigned long long *__restrict__ stats)
{
    lengths_body(src, src_off, src_len, n, only_changed, dec_len, changed, stats, PercentDecode{plus, 0u});
}

/* Payload k of the source is payload j of dst: its slot in the new arena, its decoded length, and where its bytes lie. */
__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_decode_index_kernel(const uint64_t *__restrict__ src_off, const uint32_t *__restrict__ src_len, const uint32_t *__restrict__ dec_len,
                        const uint64_t *__restrict__ loc_off, const uint32_t *__restrict__ loc_idx, const uint64_t *__restrict__ blk_bytes,
                        const uint32_t *__restrict__ blk_cnt, uint64_t n, uint64_t *__restrict__ pkt_off, uint32_t *__restrict__ pkt_len,
                        uint4 *__restrict__ recs)
{
    index_body(dec_len, loc_off, loc_idx, blk_bytes, blk_cnt, n, pkt_off, pkt_len, recs, [&](uint64_t k, uint32_t l) {
        const uint64_t so = src_off[k];
        return make_uint4((uint32_t)so, (uint32_t)(so >> 32), src_len[k], l);
    });
}

template <bool NT>
__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_decode_write_kernel(const uint8_t *__restrict__ src, const uint64_t *__restrict__ new_off, const uint4 *__restrict__ recs, uint64_t n,
                        uint64_t total, uint32_t run, uint32_t plus, uint8_t *__restrict__ dst)
{
    write_body<NT>(src, new_off, recs, n, total, run, dst, PercentDecode{plus, 0u});
}

}  // namespace

/* Phase 1: decoded lengths, changed bitmap, stats; then kmp_launch_compact_scan.  ws: kmp_extract_ws_bytes(n) bytes, kept until the index.
 * stats[3] = {source bytes, changed payloads, decoded bytes}, zeroed by the caller. */
hipError_t kmp_launch_decode_lengths(const uint8_t *src_arena, const uint64_t *src_off, const uint32_t *src_len, uint64_t n, bool plus,
                                     bool only_changed, uint8_t *ws, unsigned long long *changed, unsigned long long *stats, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(kmp_decode_lengths_kernel, dim3(kmp_group_blocks(n)), dim3(KMP_BLOCK_THREADS), 0, st, src_arena, src_off, src_len, n,
                       plus ? 1u : 0u, only_changed ? 1u : 0u, kmp_compact_ws(ws, n).len, changed, stats);
    return hipGetLastError();
}

hipError_t kmp_launch_decode_index(const uint64_t *src_off, const uint32_t *src_len, uint64_t n, uint8_t *ws, uint64_t n_dst, uint64_t *pkt_off,
                                   uint32_t *pkt_len, void *recs, hipStream_t st)
{
    if (n == 0 || n_dst == 0) return hipSuccess;
    const kmp_compact_view w = kmp_compact_ws(ws, n);
    hipLaunchKernelGGL(kmp_decode_index_kernel, dim3(kmp_item_blocks(n)), dim3(KMP_BLOCK_THREADS), 0, st, src_off, src_len, w.len, w.loc_off, w.loc_idx,
                       w.blk_bytes, w.blk_cnt, n, pkt_off, pkt_len, (uint4 *)recs);
    return hipGetLastError();
}

hipError_t kmp_launch_decode_write(const uint8_t *src_arena, const uint64_t *pkt_off, const void *recs, uint64_t n_dst, uint64_t bytes_in,
                                   uint64_t total_bytes, bool plus, uint8_t *arena, bool nontemporal, hipStream_t st)
{
    if (n_dst == 0) return hipSuccess;
    const kmp_run_shape rs = kmp_run_shape_of(n_dst, bytes_in > total_bytes ? bytes_in : total_bytes);       /* a run's SOURCE bytes count as well */
    hipLaunchKernelGGL(nontemporal ? kmp_decode_write_kernel<true> : kmp_decode_write_kernel<false>, dim3(rs.blocks), dim3(KMP_BLOCK_THREADS), 0, st,
                       src_arena, pkt_off, (const uint4 *)recs, n_dst, total_bytes, rs.run, plus ? 1u : 0u, arena);
    return hipGetLastError();
}
