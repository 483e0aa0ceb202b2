/*
 * kmp_decode.hip -- kmpgpu_load_decoded: the payloads of an arena percent-decoded on the device into a packed arena (kmpgpu.h).  gfx950.
 *
 *   kmp_decode_lengths_kernel   dec_len[k] = decoded length of payload k, or 0xFFFFFFFF ("not in dst") for an unchanged payload under
 *                               KMPGPU_DECODE_ONLY_CHANGED; the changed bitmap, one plain store per word; bytes in / out and n_changed
 *   kmp_scan_local_kernel, kmp_scan_totals_kernel   of kmp_prep.hip, through kmp_launch_repack_phase1: slot offsets and payload
 *                               numbers of dst's payloads, totals = {packed bytes, payloads}
 *   kmp_decode_index_kernel     the new index, and per payload of dst the record {source offset, source length, decoded length}
 *   kmp_decode_write_kernel     the bytes
 *
 * The transform is decided position by position (kmpgpu.h): esc(i) = p[i] == '%' and p[i+1], p[i+2] hex digits inside the payload, a
 * position is consumed where esc(i-1) or esc(i-2).  Per 16-byte unit that is bit arithmetic on three 16-bit masks ('%', hex digit,
 * inside the payload) extended by the masks of the four bytes before and after the unit; a byte at or behind the payload's end has
 * no bit in any mask, so nothing behind it decodes, whatever the slot holds there.
 *
 * Both kernels that read payload bytes deal the 16-byte units of a RUN of consecutive payloads to the lanes in order, as
 * kmp_select_copy_kernel does: lane i puts payload i of the run into the wavefront's LDS, a lane finds the payload of its unit with a
 * branch-free binary search over the run's unit prefix sums, and 64-byte payloads keep every lane as busy as 9000-byte ones.
 * Consecutive lanes hold consecutive units, so the neighbours' masks come through a lane shift; lane 0 takes the bytes before its
 * unit from the step before, and lane 63 loads the unit behind its own where its own ends in a '%'.  What a unit contributes is
 * summed per payload by a DPP scan over the wavefront and the difference to the scan value at the payload's first lane; the payload
 * that runs on into the next 64 units hands a carry on.
 *
 * The write.  A step of 64 units without any escape (or '+' under KMPGPU_DECODE_PLUS) whose output position is a multiple of 16 is a
 * straight copy: every lane stores its unit, tail cleared, where the scan says.  Any other step compacts its emitted bytes into the
 * wavefront's own LDS stage, which mirrors the destination from the last 16-byte boundary on (slots are back to back, so a step's
 * output is one contiguous range; the stage is kept all 0x00 in between, which is the padding), and goes out in whole 16-byte
 * stores; an incomplete last unit stays in the stage for the next step.  A run ends on a slot's end, so nothing is left over.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "kmp_device.h"
#include "kmp_launch.h"
#include "kmp_unit_dev.h"

namespace {

using namespace kmp_unit;     /* kmp_unit_dev.h: the units of a run dealt to the lanes, byte classes, scans, the LDS stage's sync */
typedef u32x4 dec_u32x4;

constexpr uint32_t KMP_DECODE_UNROLL = 4;             /* 16-byte units a lane has in flight */
constexpr uint32_t KMP_DECODE_LENGTHS_BLOCKS = 1024;  /* grid cap of the lengths kernel: rounds past 4 096 groups of 64 payloads */
constexpr uint32_t KMP_DECODE_INDEX_BLOCKS = 1024;    /* grid cap of the index kernel: rounds past 262 144 payloads */
constexpr uint32_t KMP_DECODE_WRITE_BLOCKS = 1024;    /* grid cap of the write kernel: rounds past 4 096 runs */
constexpr uint32_t KMP_DECODE_RUN_BYTES = 16384;      /* source bytes a run of the write should come to */
/* The stage of a step: < 16 bytes kept from the step before, <= 1024 emitted, <= 15 of padding behind each of <= 64 payloads' ends and
 * the 16-byte slots of <= 63 empty payloads in between: < 3 072. */
constexpr uint32_t KMP_DECODE_STAGE = 3072;

/* The scan workspace of kmp_prep.hip (kmp_extract_ws_bytes), as kmp_select.hip uses it: the decoded lengths take plen's place. */
struct DecodeWs {
    uint64_t *loc_off, *blk_bytes;
    uint32_t *dec_len, *loc_idx, *blk_cnt;
};
DecodeWs decode_ws(uint8_t *ws, uint64_t n)
{
    const uint64_t nblk = (n + KMP_SCAN_TILE - 1) / KMP_SCAN_TILE;
    DecodeWs w;
    w.loc_off = reinterpret_cast<uint64_t *>(ws);
    w.blk_bytes = w.loc_off + n;
    w.dec_len = reinterpret_cast<uint32_t *>(w.blk_bytes + nblk) + n;
    w.loc_idx = w.dec_len + n;
    w.blk_cnt = w.loc_idx + n;
    return w;
}

/* ---- byte classes of a dword, 0x80 in every byte of the class (eq_bytes, bits4, eq16: kmp_unit_dev.h) ---- */
__device__ __forceinline__ uint32_t hex_bytes(uint32_t w)
{
    const uint32_t lo7 = w & 0x7F7F7F7Fu;
    const uint32_t dig = (lo7 + 0x50505050u) & ~(lo7 + 0x46464646u);        /* 0x30 <= b <= 0x39 */
    const uint32_t l = lo7 | 0x20202020u;
    const uint32_t let = (l + 0x1F1F1F1Fu) & ~(l + 0x19191919u);            /* 0x61 <= b | 0x20 <= 0x66 */
    return (dig | let) & ~w & 0x80808080u;
}
__device__ __forceinline__ uint32_t hex16(dec_u32x4 v)
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
            nx = (*(const volatile __attribute__((address_space(1))) dec_u32x4 *)(uintptr_t)(addr + 16)).x;
            const uint32_t left = un.len - un.rel - 16u, vm = left >= 4u ? 0xFu : (1u << left) - 1u;
            nextm = (bits4(eq_bytes(nx, PCT4)) & vm) | (bits4(hex_bytes(nx)) & vm) << 16;
        }
    }
    if (un.rel == 0u) prevm = 0u;                               /* the lane before holds another payload's unit */
    if (un.rel + 16u >= un.len) nextm = 0u;                     /* ... and so does the lane behind */
    *next_x = nx;
    return unit_masks(own, prevm, nextm, valid);
}

__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_decode_lengths_kernel(const uint8_t *__restrict__ src, const uint64_t *__restrict__ src_off, const uint32_t *__restrict__ src_len,
                          uint64_t n, uint32_t plus, uint32_t only_changed, uint32_t *__restrict__ dec_len,
                          unsigned long long *__restrict__ changed, unsigned long long *__restrict__ stats)
{
    __shared__ uint64_t s_ub[KMP_BLOCK_WAVES][KMP_WAVE];
    __shared__ uint64_t s_src[KMP_BLOCK_WAVES][KMP_WAVE];
    __shared__ uint32_t s_len[KMP_BLOCK_WAVES][KMP_WAVE];
    __shared__ uint32_t s_dec[KMP_BLOCK_WAVES][KMP_WAVE];       /* decoded bytes of payload i so far */
    __shared__ uint32_t s_chg[KMP_BLOCK_WAVES][KMP_WAVE];
    const uint32_t lane = threadIdx.x & (KMP_WAVE - 1u), wid = threadIdx.x >> 6;
    const uint64_t n_groups = (n + KMP_WAVE - 1u) / KMP_WAVE;
    unsigned long long acc_in = 0ull, acc_out = 0ull, acc_chg = 0ull;
    for (uint64_t r = (uint64_t)blockIdx.x * KMP_BLOCK_WAVES + wid; r < n_groups; r += (uint64_t)gridDim.x * KMP_BLOCK_WAVES) {
        const uint64_t k = r * KMP_WAVE + lane;
        const bool in = k < n;
        const uint32_t len = in ? src_len[k] : 0u;
        const uint64_t so = in ? src_off[k] : 0ull;
        const uint64_t units = ((uint64_t)len + 15u) >> 4;
        const uint64_t incl = wave_incl_scan64(units, lane);
        const uint64_t total_units = bcast64(incl, KMP_WAVE - 1u);
        __builtin_amdgcn_wave_barrier();
        s_ub[wid][lane] = incl - units; s_src[wid][lane] = so; s_len[wid][lane] = len; s_dec[wid][lane] = 0u; s_chg[wid][lane] = 0u;
        lds_wave_sync();
        uint32_t tail_w = 0u;                                   /* the last four bytes of the step before */
        for (uint64_t g0 = 0; g0 < total_units; g0 += (uint64_t)KMP_DECODE_UNROLL * KMP_WAVE) {
            Unit un[KMP_DECODE_UNROLL];
#pragma unroll
            for (uint32_t u = 0; u < KMP_DECODE_UNROLL; ++u)
                load_step<false>(un[u], src, s_ub[wid], s_src[wid], s_len[wid], g0 + (uint64_t)u * KMP_WAVE, total_units, lane);
#pragma unroll
            for (uint32_t u = 0; u < KMP_DECODE_UNROLL; ++u) {
                const uint64_t gs = g0 + (uint64_t)u * KMP_WAVE;
                if (gs >= total_units) break;
                const Unit &q = un[u];
                const uint32_t valid = q.act ? valid_bits(q.len - q.rel) : 0u;
                const uint32_t hp = (lane == 0u && q.rel) ? tail_w : 0u;
                tail_w = (uint32_t)__builtin_amdgcn_readlane((int)q.v.w, 63);
                const uint32_t P16 = eq16(q.v, PCT4) & valid;
                const uint32_t plus16 = plus ? eq16(q.v, PLUS4) & valid : 0u;
                uint32_t cnt = __popc(valid);
                bool chg = plus16 != 0u;
                if (__any(P16 | (bits4(eq_bytes(hp, PCT4)) & 0xCu))) {
                    uint32_t nx;
                    const UnitMasks m = step_masks(q, hp, src + s_src[wid][q.p] + q.rel, lane, valid, P16, &nx);
                    cnt = __popc(m.emit);
                    chg = chg || m.emit != valid;
                }
                /* the step's bytes of each payload, added by the lane that holds the payload's last unit of the step */
                const uint32_t s_incl = wave_incl_scan(cnt);
                const uint32_t base = __shfl(s_incl - cnt, (int)q.first);
                if (q.act) {
                    if (chg) s_chg[wid][q.p] = 1u;
                    if (lane == KMP_WAVE - 1u || gs + lane + 1u >= total_units || q.rel + 16u >= q.len) s_dec[wid][q.p] += s_incl - base;
                }
                lds_wave_sync();
            }
        }
        lds_wave_sync();
        const uint32_t dec = s_dec[wid][lane];
        const bool chg = in && s_chg[wid][lane] != 0u;
        const bool held = in && (chg || !only_changed);
        const unsigned long long word = __ballot(chg);
        if (in) dec_len[k] = held ? dec : 0xFFFFFFFFu;
        if (lane == 0u) changed[r] = word;                      /* one word per wavefront: bits at n and above are 0 */
        acc_in += held ? len : 0u; acc_out += held ? dec : 0u; acc_chg += chg ? 1u : 0u;
        __builtin_amdgcn_wave_barrier();
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { acc_in += __shfl_xor(acc_in, o); acc_out += __shfl_xor(acc_out, o); acc_chg += __shfl_xor(acc_chg, o); }
    if (lane == 0u) {
        if (acc_in) atomicAdd(stats + 0, acc_in);
        if (acc_chg) atomicAdd(stats + 1, acc_chg);
        if (acc_out) atomicAdd(stats + 2, acc_out);
    }
}

/* Payload k of the source is payload j of dst: its slot in the new arena, its decoded length, and where its bytes lie. */
__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_decode_index_kernel(const uint64_t *__restrict__ src_off, const uint32_t *__restrict__ src_len, const uint32_t *__restrict__ dec_len,
                        const uint64_t *__restrict__ loc_off, const uint32_t *__restrict__ loc_idx, const uint64_t *__restrict__ blk_bytes,
                        const uint32_t *__restrict__ blk_cnt, uint64_t n, uint64_t *__restrict__ pkt_off, uint32_t *__restrict__ pkt_len,
                        uint4 *__restrict__ recs)
{
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t l = dec_len[k];
        if (l == 0xFFFFFFFFu) continue;
        const uint64_t blk = k / KMP_SCAN_TILE;
        const uint64_t j = (uint64_t)blk_cnt[blk] + loc_idx[k];
        const uint64_t so = src_off[k];
        pkt_off[j] = blk_bytes[blk] + loc_off[k];
        pkt_len[j] = l;
        recs[j] = make_uint4((uint32_t)so, (uint32_t)(so >> 32), src_len[k], l);
    }
}

__device__ __forceinline__ uint32_t hex_val(uint32_t c) { return (c & 0xFu) + (c >> 6) * 9u; }

template <bool NT>
__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_decode_write_kernel(const uint8_t *__restrict__ src, const uint64_t *__restrict__ new_off, const uint4 *__restrict__ recs, uint64_t n,
                        uint64_t total, uint32_t run, uint32_t plus, uint8_t *__restrict__ dst)
{
    __shared__ uint64_t s_ub[KMP_BLOCK_WAVES][KMP_WAVE];
    __shared__ uint64_t s_src[KMP_BLOCK_WAVES][KMP_WAVE];
    __shared__ uint64_t s_off[KMP_BLOCK_WAVES][KMP_WAVE];       /* new offset of payload i of the run */
    __shared__ uint32_t s_len[KMP_BLOCK_WAVES][KMP_WAVE];
    __shared__ dec_u32x4 s_stage[KMP_BLOCK_WAVES][KMP_DECODE_STAGE / 16u];
    const uint32_t lane = threadIdx.x & (KMP_WAVE - 1u), wid = threadIdx.x >> 6;
    dec_u32x4 *stage = s_stage[wid];
    uint8_t *stage_b = reinterpret_cast<uint8_t *>(stage);
    for (uint32_t q = lane; q < KMP_DECODE_STAGE / 16u; q += KMP_WAVE) stage[q] = (dec_u32x4)(0u);
    const uint64_t n_runs = (n + run - 1u) / run;
    for (uint64_t r = (uint64_t)blockIdx.x * KMP_BLOCK_WAVES + wid; r < n_runs; r += (uint64_t)gridDim.x * KMP_BLOCK_WAVES) {
        const uint64_t j = r * run + lane;
        const bool in = lane < run && j < n;
        uint64_t off = 0ull, so = 0ull;
        uint32_t len = 0u;
        if (in) {
            const uint4 rec = recs[j];
            off = new_off[j];
            so = ((uint64_t)rec.y << 32) | rec.x;
            len = rec.z;
            if (rec.w == 0u && off + 16u <= total) store_unit<NT>(dst + off, (dec_u32x4)(0u));      /* an empty payload's zero slot */
        }
        const uint64_t units = ((uint64_t)len + 15u) >> 4;
        const uint64_t incl = wave_incl_scan64(units, lane);
        const uint64_t total_units = bcast64(incl, KMP_WAVE - 1u);
        __builtin_amdgcn_wave_barrier();
        s_ub[wid][lane] = incl - units; s_src[wid][lane] = so; s_off[wid][lane] = off; s_len[wid][lane] = len;
        lds_wave_sync();
        uint32_t tail_w = 0u;                                   /* the last four bytes of the step before */
        uint32_t carry = 0u;                                    /* decoded bytes of the payload that runs on into the step, before it */
        for (uint64_t g0 = 0; g0 < total_units; g0 += (uint64_t)KMP_DECODE_UNROLL * KMP_WAVE) {
            Unit un[KMP_DECODE_UNROLL];
#pragma unroll
            for (uint32_t u = 0; u < KMP_DECODE_UNROLL; ++u)
                load_step<NT>(un[u], src, s_ub[wid], s_src[wid], s_len[wid], g0 + (uint64_t)u * KMP_WAVE, total_units, lane);
#pragma unroll
            for (uint32_t u = 0; u < KMP_DECODE_UNROLL; ++u) {
                const uint64_t gs = g0 + (uint64_t)u * KMP_WAVE;
                if (gs >= total_units) break;
                const Unit &q = un[u];
                const uint32_t last_lane = (uint32_t)min((uint64_t)(KMP_WAVE - 1u), total_units - 1u - gs);
                const uint32_t valid = q.act ? valid_bits(q.len - q.rel) : 0u;
                const uint32_t hp = (lane == 0u && q.rel) ? tail_w : 0u;
                tail_w = (uint32_t)__builtin_amdgcn_readlane((int)q.v.w, 63);
                const uint32_t P16 = eq16(q.v, PCT4) & valid;
                const uint32_t plus16 = plus ? eq16(q.v, PLUS4) & valid : 0u;
                const bool ends = q.rel + 16u >= q.len;         /* the payload's last unit */
                const uint64_t doff = s_off[wid][q.p];
                uint32_t next_carry;
                if (!__any(P16 | plus16 | (bits4(eq_bytes(hp, PCT4)) & 0xCu)) && (carry & 15u) == 0u) {
                    /* nothing to decode and 16-byte aligned: the units go out as they are, tails cleared */
                    const uint32_t before = q.started ? carry + 16u * lane : q.rel;
                    const uint64_t d = doff + before;
                    if (q.act && d + 16u <= total) store_unit<NT>(dst + d, keep_bytes(q.v, q.len - q.rel));
                    next_carry = ends ? 0u : before + 16u;
                } else {
                    uint32_t nx;
                    const UnitMasks m = step_masks(q, hp, src + s_src[wid][q.p] + q.rel, lane, valid, P16, &nx);
                    const uint32_t cnt = __popc(m.emit);
                    const uint32_t s_incl = wave_incl_scan(cnt);
                    const uint32_t base = __shfl(s_incl - cnt, (int)q.first);
                    const uint32_t before = s_incl - cnt - base + (q.started ? carry : 0u);
                    const uint64_t out = doff + before;
                    const uint64_t a0 = bcast64(out, 0u) & ~15ull;                  /* the stage's place in dst */
                    uint32_t pos = q.act ? (uint32_t)(out - a0) : 0u;
                    const uint32_t w[5] = {q.v.x, q.v.y, q.v.z, q.v.w, nx};
#pragma unroll
                    for (uint32_t i = 0; i < 16u; ++i) {
                        if ((m.emit >> i) & 1u) {
                            uint32_t b = (w[i >> 2] >> (8u * (i & 3u))) & 0xFFu;
                            if ((m.esc >> i) & 1u)
                                b = hex_val((w[(i + 1u) >> 2] >> (8u * ((i + 1u) & 3u))) & 0xFFu) << 4 |
                                    hex_val((w[(i + 2u) >> 2] >> (8u * ((i + 2u) & 3u))) & 0xFFu);
                            else if ((plus16 >> i) & 1u) b = 0x20u;
                            if (pos < KMP_DECODE_STAGE) stage_b[pos] = (uint8_t)b;
                            ++pos;
                        }
                    }
                    const uint32_t end_l = ends ? (pos + 15u) & ~15u : pos;          /* a payload's end completes its slot with the stage's 0x00 */
                    const uint32_t end = min((uint32_t)__shfl(end_l, (int)last_lane), KMP_DECODE_STAGE);
                    const uint32_t n_full = end >> 4;
                    lds_wave_sync();
                    for (uint32_t t = lane; t < n_full; t += KMP_WAVE) {
                        const uint64_t d = a0 + 16ull * t;
                        if (d + 16u <= total) store_unit<NT>(dst + d, stage[t]);
                    }
                    const bool rest = (end & 15u) != 0u && n_full < KMP_DECODE_STAGE / 16u;
                    const dec_u32x4 part = rest ? stage[n_full] : (dec_u32x4)(0u);
                    lds_wave_sync();
                    for (uint32_t t = lane; t < (end + 15u) >> 4; t += KMP_WAVE) stage[t] = (dec_u32x4)(0u);
                    lds_wave_sync();
                    if (rest && lane == 0u) stage[0] = part;                         /* the next step begins inside this unit */
                    lds_wave_sync();
                    next_carry = ends ? 0u : before + cnt;
                }
                carry = __builtin_amdgcn_readfirstlane(__shfl(next_carry, (int)last_lane));
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

}  // namespace

/* Phase 1: decoded lengths, changed bitmap, stats + scan; totals[0] = bytes of the packed result, totals[1] = its payloads.  ws:
 * kmp_extract_ws_bytes(n) bytes, kept until phase 2.  stats[3] = {source bytes, changed payloads, decoded bytes}, zeroed by the caller. */
hipError_t kmp_launch_decode_lengths(const uint8_t *src_arena, const uint64_t *src_off, const uint32_t *src_len, uint64_t n, bool plus,
                                     bool only_changed, uint8_t *ws, unsigned long long *changed, unsigned long long *stats, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    const DecodeWs w = decode_ws(ws, n);
    const uint64_t groups = (n + KMP_WAVE - 1) / KMP_WAVE;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((groups + KMP_BLOCK_WAVES - 1) / KMP_BLOCK_WAVES, KMP_DECODE_LENGTHS_BLOCKS);
    hipLaunchKernelGGL(kmp_decode_lengths_kernel, dim3(blocks), dim3(KMP_BLOCK_THREADS), 0, st, src_arena, src_off, src_len, n, plus ? 1u : 0u,
                       only_changed ? 1u : 0u, w.dec_len, changed, stats);
    return hipGetLastError();
}

hipError_t kmp_launch_decode_scan(uint64_t n, uint8_t *ws, unsigned long long *totals, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    return kmp_launch_repack_phase1(decode_ws(ws, n).dec_len, n, ws, totals, st);       /* kmp_scan_local_kernel + kmp_scan_totals_kernel */
}

hipError_t kmp_launch_decode_index(const uint64_t *src_off, const uint32_t *src_len, uint64_t n, uint8_t *ws, uint64_t n_dst, uint64_t *pkt_off,
                                   uint32_t *pkt_len, void *recs, hipStream_t st)
{
    if (n == 0 || n_dst == 0) return hipSuccess;
    const DecodeWs w = decode_ws(ws, n);
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((n + KMP_BLOCK_THREADS - 1) / KMP_BLOCK_THREADS, KMP_DECODE_INDEX_BLOCKS);
    hipLaunchKernelGGL(kmp_decode_index_kernel, dim3(blocks), dim3(KMP_BLOCK_THREADS), 0, st, src_off, src_len, w.dec_len, w.loc_off, w.loc_idx,
                       w.blk_bytes, w.blk_cnt, n, pkt_off, pkt_len, (uint4 *)recs);
    return hipGetLastError();
}

hipError_t kmp_launch_decode_write(const uint8_t *src_arena, const uint64_t *pkt_off, const void *recs, uint64_t n_dst, uint64_t bytes_in,
                                   uint64_t total_bytes, bool plus, uint8_t *arena, bool nontemporal, hipStream_t st)
{
    if (n_dst == 0) return hipSuccess;
    /* payloads per run: what brings an average run to KMP_DECODE_RUN_BYTES of source, a power of two up to 64 */
    const uint64_t avg = std::max<uint64_t>(std::max(bytes_in, total_bytes) / n_dst, 16);
    uint32_t run = KMP_WAVE;
    while (run > 1u && (uint64_t)run * avg > KMP_DECODE_RUN_BYTES) run >>= 1;
    const uint64_t n_runs = (n_dst + run - 1) / run;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((n_runs + KMP_BLOCK_WAVES - 1) / KMP_BLOCK_WAVES, KMP_DECODE_WRITE_BLOCKS);
    if (nontemporal)
        hipLaunchKernelGGL(kmp_decode_write_kernel<true>, dim3(blocks), dim3(KMP_BLOCK_THREADS), 0, st, src_arena, pkt_off, (const uint4 *)recs,
                           n_dst, total_bytes, run, plus ? 1u : 0u, arena);
    else
        hipLaunchKernelGGL(kmp_decode_write_kernel<false>, dim3(blocks), dim3(KMP_BLOCK_THREADS), 0, st, src_arena, pkt_off, (const uint4 *)recs,
                           n_dst, total_bytes, run, plus ? 1u : 0u, arena);
    return hipGetLastError();
}
