/*
 * kmp_compact_dev.h -- the one skeleton of the builders that compact payloads into a derived, packed arena: kmp_select.hip, kmp_decode.hip,
 * kmp_base64.hip, kmp_fields.hip and kmp_seams.hip ("The compacting skeleton").  Device code only; gfx950.
 *
 * Every builder runs the same four steps over the scan workspace (kmp_compact_ws, kmp_launch.h):
 *   lengths   len[k] of payload k in the destination, or 0xFFFFFFFF ("not in dst").  Where the length is only known from the payload's
 *             bytes: lengths_body.  Where a bitmap and three sums go with it: group_tail, group_sums_flush.
 *   scan      kmp_launch_compact_scan: slot offsets and payload numbers.
 *   index     index_body: pkt_off, pkt_len and one 16-byte record per payload of the destination; the kernel says what the record holds.
 *   write     a wavefront takes a RUN of consecutive destination payloads (kmp_run_shape_of), tables them in its own LDS, deals 16-byte
 *             units to the lanes in order and finds a unit's payload by a branch-free binary search (find_payload), so that 64-byte
 *             payloads keep every lane as busy as 9000-byte ones and the stores are contiguous whatever the payload boundaries.
 *             gather_runs deals the DESTINATION's units: the slots' offsets are the prefix sums, nothing is summed, and the kernel
 *             says where the 16 bytes at (payload, offset) come from.  write_body deals the SOURCE's units, because what a unit yields
 *             is known only from its bytes: a policy says which bytes a unit emits and what they are, and the body sums per payload,
 *             stores a step that changes nothing as it is and compacts any other step through the wavefront's LDS stage.
 *
 * A wavefront's LDS is its own here: its DS instructions execute in order, and wave barriers keep the compiler from moving them.
 */
#ifndef KMP_COMPACT_DEV_H
#define KMP_COMPACT_DEV_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kmp_device.h"
#include "kmp_launch.h"
#include "kmp_unit_dev.h"

namespace kmp_unit {

constexpr uint32_t KMP_NOT_IN_DST = 0xFFFFFFFFu;

/* ---- index: item k of the source is payload j of the destination.  rec(k, l) -> the uint4 the write kernel reads for it. ---- */
template <class Rec>
static __device__ __forceinline__ void index_body(const uint32_t *len, const uint64_t *loc_off, const uint32_t *loc_idx, const uint64_t *blk_bytes,
                                                  const uint32_t *blk_cnt, uint64_t n, uint64_t *pkt_off, uint32_t *pkt_len, uint4 *recs, Rec rec)
{
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t l = len[k];
        if (l == KMP_NOT_IN_DST) continue;
        const uint64_t blk = k / KMP_SCAN_TILE;
        const uint64_t j = (uint64_t)blk_cnt[blk] + loc_idx[k];
        const uint4 r = rec(k, l);
        pkt_off[j] = blk_bytes[blk] + loc_off[k];
        pkt_len[j] = l;
        recs[j] = r;
    }
}

/* ---- the tail of a lengths kernel's group of 64 items: the length, the group's word of the flag bitmap (bits at n and above are 0), and
 * the three sums {source bytes of the items held, flagged items, destination bytes} that go to stats[3] once per wavefront ---- */
struct GroupSums { unsigned long long in, flagged, out; };
static __device__ __forceinline__ void group_tail(GroupSums &acc, bool in, uint64_t k, uint64_t group, uint32_t lane, bool flag, bool only_flagged,
                                                  uint32_t src_len, uint32_t dst_len, uint32_t *len, unsigned long long *bitmap)
{
    flag = in && flag;
    const bool held = in && (flag || !only_flagged);
    const unsigned long long word = __ballot(flag);
    if (in) len[k] = held ? dst_len : KMP_NOT_IN_DST;
    if (lane == 0u) bitmap[group] = word;                       /* one plain store per word */
    acc.in += held ? src_len : 0u; acc.out += held ? dst_len : 0u; acc.flagged += flag ? 1u : 0u;
}
static __device__ __forceinline__ void group_sums_flush(GroupSums acc, uint32_t lane, unsigned long long *stats)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { acc.in += __shfl_xor(acc.in, o); acc.out += __shfl_xor(acc.out, o); acc.flagged += __shfl_xor(acc.flagged, o); }
    if (lane == 0u) {
        if (acc.in) atomicAdd(stats + 0, acc.in);
        if (acc.flagged) atomicAdd(stats + 1, acc.flagged);
        if (acc.out) atomicAdd(stats + 2, acc.out);
    }
}

/* ---- write, by destination units.  load(j, in) -> the record of payload j = j0 + i of the run in lane i (in: there is such a payload),
 * asked for together with the payload's offset and in front of the barrier, so that a run waits for memory once; table(rec): the lane puts
 * it into the kernel's own LDS rows.  fetch(p, rel, keep) -> the 16 bytes at offset rel of payload p of the run, 0 for an empty payload's
 * slot; keep: how many of them count where that is fewer than 16 -- the rest is cleared at the store, so that no ALU instruction waits
 * for a load while the lane's other units are still to be asked for.  UNROLL units per lane are in flight. ---- */
template <bool NT, uint32_t UNROLL, class Load, class Table, class Fetch>
static __device__ __forceinline__ void gather_runs(const uint64_t *new_off, uint64_t n, uint64_t total, uint32_t run, uint8_t *dst, Load load,
                                                   Table table, Fetch fetch)
{
    __shared__ uint64_t s_off[KMP_BLOCK_WAVES][KMP_WAVE];          /* new offset of payload i of the run; ~0 behind the run's end */
    const uint32_t lane = threadIdx.x & (KMP_WAVE - 1u), wid = threadIdx.x >> 6;
    const uint64_t n_runs = (n + run - 1u) / run;
    for (uint64_t r = (uint64_t)blockIdx.x * KMP_BLOCK_WAVES + wid; r < n_runs; r += (uint64_t)gridDim.x * KMP_BLOCK_WAVES) {
        const uint64_t j0 = r * run, j = j0 + lane;
        const bool in = lane < run && j < n;
        const uint64_t off = in ? new_off[j] : ~0ull;
        const auto rec = load(j, in);
        __builtin_amdgcn_wave_barrier();
        s_off[wid][lane] = off;
        table(rec);
        lds_wave_sync();
        const uint64_t base = new_off[j0];
        const uint64_t end = (j0 + run < n) ? new_off[j0 + run] : total;
        for (uint64_t d0 = base + (uint64_t)lane * 16u; d0 - lane * 16u < end; d0 += (uint64_t)UNROLL * KMP_WAVE * 16u) {
            u32x4 v[UNROLL];
            uint32_t keep[UNROLL];
#pragma unroll
            for (uint32_t u = 0; u < UNROLL; ++u) {
                const uint64_t d = d0 + (uint64_t)u * KMP_WAVE * 16u;
                v[u] = (u32x4)(0u);
                keep[u] = 16u;
                if (d < end) {
                    const uint32_t p = find_payload(s_off[wid], d);
                    v[u] = fetch(p, d - s_off[wid][p], keep[u]);
                }
            }
#pragma unroll
            for (uint32_t u = 0; u < UNROLL; ++u) {
                const uint64_t d = d0 + (uint64_t)u * KMP_WAVE * 16u;
                if (d < end) store_unit<NT>(dst + d, keep_bytes(v[u], keep[u]));
            }
        }
        __builtin_amdgcn_wave_barrier();                             /* the next run's table goes over this one */
    }
}

/* ---- lengths and write, by source units: the transforms that emit a subset of a payload's positions, each as one byte.
 *
 * A Policy holds the transform's parameters and what one step of 64 units hands to the next, and has
 *   void  reset()                        at a run's first step
 *   Step  step(q, addr, lane)            all 64 lanes, once per step and in order.  q: the lane's unit, addr: where it lies.  Step has
 *                                        valid (the positions inside the payload), emit (those that yield a byte) and changed (the unit
 *                                        makes its payload differ from the source), and whatever byte() needs.  A test that lets a
 *                                        step without anything to decode off cheaply is the policy's own, and wave-uniform.
 *   uint32_t byte(st, q, i)              the byte position i yields; called for i = 0 .. 15 in turn, st may keep a running state
 * A step whose units all emit every position and change nothing, at an output position that is a multiple of 16, is stored as it is. ---- */
constexpr uint32_t KMP_UNIT_UNROLL = 4;             /* steps a lane has in flight */
/* The stage of a step: < 16 bytes kept from the step before, <= 1024 emitted (no transform yields more bytes than it reads), <= 15 of
 * padding behind each of <= 64 payloads' ends and the 16-byte slots of <= 63 empty payloads in between: < 3 072. */
constexpr uint32_t KMP_STAGE_BYTES = 3072;

template <class Policy>
static __device__ __forceinline__ void lengths_body(const uint8_t *src, const uint64_t *src_off, const uint32_t *src_len, uint64_t n, uint32_t only_changed,
                                                    uint32_t *dec_len, unsigned long long *changed, unsigned long long *stats, Policy P)
{
    __shared__ uint64_t s_ub[KMP_BLOCK_WAVES][KMP_WAVE];
    __shared__ uint64_t s_src[KMP_BLOCK_WAVES][KMP_WAVE];
    __shared__ uint32_t s_len[KMP_BLOCK_WAVES][KMP_WAVE];
    __shared__ uint32_t s_dec[KMP_BLOCK_WAVES][KMP_WAVE];       /* bytes payload i yields so far */
    __shared__ uint32_t s_chg[KMP_BLOCK_WAVES][KMP_WAVE];
    const uint32_t lane = threadIdx.x & (KMP_WAVE - 1u), wid = threadIdx.x >> 6;
    const uint64_t n_groups = (n + KMP_WAVE - 1u) / KMP_WAVE;
    GroupSums acc = {0ull, 0ull, 0ull};
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
        P.reset();
        for (uint64_t g0 = 0; g0 < total_units; g0 += (uint64_t)KMP_UNIT_UNROLL * KMP_WAVE) {
            Unit un[KMP_UNIT_UNROLL];
#pragma unroll
            for (uint32_t u = 0; u < KMP_UNIT_UNROLL; ++u)
                load_step<false>(un[u], src, s_ub[wid], s_src[wid], s_len[wid], g0 + (uint64_t)u * KMP_WAVE, total_units, lane);
#pragma unroll
            for (uint32_t u = 0; u < KMP_UNIT_UNROLL; ++u) {
                const uint64_t gs = g0 + (uint64_t)u * KMP_WAVE;
                if (gs >= total_units) break;
                const Unit &q = un[u];
                const auto st = P.step(q, src + s_src[wid][q.p] + q.rel, lane);
                const uint32_t cnt = __popc(st.emit);
                /* the step's bytes of each payload, added by the lane that holds the payload's last unit of the step */
                const uint32_t s_incl = wave_incl_scan(cnt);
                const uint32_t base = __shfl(s_incl - cnt, (int)q.first);
                if (q.act) {
                    if (st.changed) s_chg[wid][q.p] = 1u;
                    if (lane == KMP_WAVE - 1u || gs + lane + 1u >= total_units || q.rel + 16u >= q.len) s_dec[wid][q.p] += s_incl - base;
                }
                lds_wave_sync();
            }
        }
        lds_wave_sync();
        group_tail(acc, in, k, r, lane, s_chg[wid][lane] != 0u, only_changed != 0u, len, s_dec[wid][lane], dec_len, changed);
        __builtin_amdgcn_wave_barrier();
    }
    group_sums_flush(acc, lane, stats);
}

/* recs[j] = {source offset (64 bits), source length, length in dst}, new_off[j]: the slot; a run ends on a slot's end, so the stage is
 * empty again there. */
template <bool NT, class Policy>
static __device__ __forceinline__ void write_body(const uint8_t *src, const uint64_t *new_off, const uint4 *recs, uint64_t n, uint64_t total, uint32_t run,
                                                  uint8_t *dst, Policy P)
{
    __shared__ uint64_t s_ub[KMP_BLOCK_WAVES][KMP_WAVE];
    __shared__ uint64_t s_src[KMP_BLOCK_WAVES][KMP_WAVE];
    __shared__ uint64_t s_off[KMP_BLOCK_WAVES][KMP_WAVE];       /* new offset of payload i of the run */
    __shared__ uint32_t s_len[KMP_BLOCK_WAVES][KMP_WAVE];
    /* mirrors the destination from the last 16-byte boundary on (slots are back to back, so a step's output is one contiguous range) and
     * is kept all 0x00 in between, which is the padding */
    __shared__ u32x4 s_stage[KMP_BLOCK_WAVES][KMP_STAGE_BYTES / 16u];
    const uint32_t lane = threadIdx.x & (KMP_WAVE - 1u), wid = threadIdx.x >> 6;
    u32x4 *stage = s_stage[wid];
    uint8_t *stage_b = reinterpret_cast<uint8_t *>(stage);
    for (uint32_t q = lane; q < KMP_STAGE_BYTES / 16u; q += KMP_WAVE) stage[q] = (u32x4)(0u);
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
            if (rec.w == 0u && off + 16u <= total) store_unit<NT>(dst + off, (u32x4)(0u));      /* an empty payload's zero slot */
        }
        const uint64_t units = ((uint64_t)len + 15u) >> 4;
        const uint64_t incl = wave_incl_scan64(units, lane);
        const uint64_t total_units = bcast64(incl, KMP_WAVE - 1u);
        __builtin_amdgcn_wave_barrier();
        s_ub[wid][lane] = incl - units; s_src[wid][lane] = so; s_off[wid][lane] = off; s_len[wid][lane] = len;
        lds_wave_sync();
        P.reset();
        uint32_t carry = 0u;                                    /* bytes the payload that runs on into the step has yielded before it */
        for (uint64_t g0 = 0; g0 < total_units; g0 += (uint64_t)KMP_UNIT_UNROLL * KMP_WAVE) {
            Unit un[KMP_UNIT_UNROLL];
#pragma unroll
            for (uint32_t u = 0; u < KMP_UNIT_UNROLL; ++u)
                load_step<NT>(un[u], src, s_ub[wid], s_src[wid], s_len[wid], g0 + (uint64_t)u * KMP_WAVE, total_units, lane);
#pragma unroll
            for (uint32_t u = 0; u < KMP_UNIT_UNROLL; ++u) {
                const uint64_t gs = g0 + (uint64_t)u * KMP_WAVE;
                if (gs >= total_units) break;
                const Unit &q = un[u];
                const uint32_t last_lane = (uint32_t)min((uint64_t)(KMP_WAVE - 1u), total_units - 1u - gs);
                const bool ends = q.rel + 16u >= q.len;         /* the payload's last unit */
                const uint64_t doff = s_off[wid][q.p];
                auto st = P.step(q, src + s_src[wid][q.p] + q.rel, lane);
                uint32_t next_carry;
                if (!__any(st.changed || st.emit != st.valid) && (carry & 15u) == 0u) {
                    /* nothing to transform and 16-byte aligned: the units go out as they are, tails cleared */
                    const uint32_t before = q.started ? carry + 16u * lane : q.rel;
                    const uint64_t d = doff + before;
                    if (q.act && d + 16u <= total) store_unit<NT>(dst + d, keep_bytes(q.v, q.len - q.rel));
                    next_carry = ends ? 0u : before + 16u;
                } else {
                    const uint32_t cnt = __popc(st.emit);
                    const uint32_t s_incl = wave_incl_scan(cnt);
                    const uint32_t base = __shfl(s_incl - cnt, (int)q.first);
                    const uint32_t before = s_incl - cnt - base + (q.started ? carry : 0u);
                    const uint64_t out = doff + before;
                    const uint64_t a0 = bcast64(out, 0u) & ~15ull;                  /* the stage's place in dst */
                    uint32_t pos = q.act ? (uint32_t)(out - a0) : 0u;
#pragma unroll
                    for (uint32_t i = 0; i < 16u; ++i) {
                        const uint32_t b = P.byte(st, q, i);
                        if ((st.emit >> i) & 1u) {
                            if (pos < KMP_STAGE_BYTES) stage_b[pos] = (uint8_t)b;
                            ++pos;
                        }
                    }
                    const uint32_t end_l = ends ? (pos + 15u) & ~15u : pos;          /* a payload's end completes its slot with the stage's 0x00 */
                    const uint32_t end = min((uint32_t)__shfl(end_l, (int)last_lane), KMP_STAGE_BYTES);
                    const uint32_t n_full = end >> 4;
                    lds_wave_sync();
                    for (uint32_t t = lane; t < n_full; t += KMP_WAVE) {
                        const uint64_t d = a0 + 16ull * t;
                        if (d + 16u <= total) store_unit<NT>(dst + d, stage[t]);
                    }
                    const bool rest = (end & 15u) != 0u && n_full < KMP_STAGE_BYTES / 16u;
                    const u32x4 part = rest ? stage[n_full] : (u32x4)(0u);
                    lds_wave_sync();
                    for (uint32_t t = lane; t < (end + 15u) >> 4; t += KMP_WAVE) stage[t] = (u32x4)(0u);
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

}  // namespace kmp_unit

#endif
