/*
 * kmp_flows.hip -- flows on gfx950 (kmpgpu_flows_build, kmpgpu_scan_flows, kmpgpu_flows_select; kmpgpu.h): the payloads of an arena grouped
 * by the 5-tuple of their metadata records, the hit matrix folded from payload space into flow space, and a flow bitmap expanded back.
 *
 *   kmp_flows_insert_kernel   every payload's key into an open-addressing table of 32-bit slots (payload index + 1, 0 = empty); slot_of[k],
 *                             first[slot] = the lowest payload index of the slot's flow
 *   kmp_flows_firsts_kernel   is_first[k] = (first[slot_of[k]] == k), written as the "length" the scan kernels of kmp_prep.hip take (16 for
 *                             a first payload, 0xFFFFFFFF "rejected" otherwise), as kmp_alerts.hip writes its counts
 *   kmp_scan_local_kernel, kmp_scan_totals_kernel   of kmp_prep.hip, through kmp_launch_compact_scan: a first payload's rank among the
 *                             first payloads = its flow's id, totals[1] = n_flows
 *   kmp_flows_number_kernel   a first payload writes its flow's id over its slot of the table and opens the flow's record
 *   kmp_flows_assign_kernel   flow_of[k] = table[slot_of[k]] (in place, over slot_of); n_packets, payload_bytes, last_packet of the records
 *   kmp_flows_fold_kernel     out[r][f] |= rows[r][k] for f = flow_of[k]
 *   kmp_flows_expand_kernel   pkt[k] = flow_bits[flow_of[k]]
 *
 * Everywhere a lane owns a payload and a wavefront 64 consecutive ones, as in kmp_headers.hip; the record is one 16-byte load.
 *
 * Nothing depends on the run.  Which payload wins the compare-and-swap on an empty slot does: but the table is only ever read as "the slot
 * names SOME payload of this flow" (the keys are compared, and all payloads of a flow have one key), and which slot a flow ends up in --
 * which also depends on the race, where two flows probe through one another -- is never an output.  The flow's first payload is a minimum,
 * its id a rank in payload order, its counters sums and a maximum.
 *
 * Atomics.  One address takes about 88 atomics per microsecond on this chip, and a capture of a million payloads that is ONE flow (the
 * synthetic benchmark arena) would pay 11 ms for a per-payload atomic on one word.  So every atomic here is issued once per distinct
 * target per wavefront: the lanes that share a target are found with a ballot loop over the wavefront's distinct targets (one round when
 * the wavefront is one flow, 64 at worst), their values are combined across the lanes, and the group's first lane issues the atomic.  In
 * the insert the groups are the lanes of one key, and only a group's first lane goes to the table at all: its compare-and-swap is tried
 * only on a slot just read as empty, so a hot flow's slot is swapped at most once per wavefront that meets it empty and read ever after.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "kmpgpu.h"
#include "kmp_device.h"
#include "kmp_flow_key.h"
#include "kmp_launch.h"

namespace {

constexpr uint32_t FLOW_THREADS = 256u;
constexpr uint32_t FLOW_WAVES = FLOW_THREADS / KMP_WAVE;
constexpr uint32_t FLOW_REC_WORDS = 6u;         /* 64-bit words of a kmpgpu_flow: first_packet, last_packet, n_packets, payload_bytes, first (two) */
constexpr uint32_t FLOW_FOLD_MAX_BY = 64u;

__device__ __forceinline__ uint32_t lane_value(uint32_t v, uint32_t lane) { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)lane); }

__device__ __forceinline__ uint64_t shfl_xor64(uint64_t v, uint32_t s)
{
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, (int)s), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), (int)s);
    return ((uint64_t)hi << 32) | lo;
}
/* over all 64 lanes (a lane outside the group brings 0); every lane gets the result */
__device__ __forceinline__ uint64_t wave_sum64(uint64_t v)
{
#pragma unroll
    for (uint32_t s = 32u; s; s >>= 1) v += shfl_xor64(v, s);
    return v;
}
__device__ __forceinline__ uint64_t wave_or64(uint64_t v)
{
#pragma unroll
    for (uint32_t s = 32u; s; s >>= 1) v |= shfl_xor64(v, s);
    return v;
}

__global__ void __launch_bounds__(FLOW_THREADS)
kmp_flows_insert_kernel(const uint4 *__restrict__ meta, uint64_t n_pkts, uint32_t directed, uint32_t *table, uint32_t mask,
                        uint32_t *__restrict__ first, uint32_t *__restrict__ slot_of)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t k = (uint64_t)blockIdx.x * FLOW_THREADS + threadIdx.x;
    const bool live = k < n_pkts;
    kmp_flow_key key = {0ull, 0ull, 0u};
    if (live) {
        const uint4 M = meta[k];
        key = kmp_flow_key_of(M.x, M.y, M.z, M.w, directed != 0u);
    }
    /* The lanes of the wavefront that share a key: the lowest of them, their head, probes for all -- one round per distinct key.  A
     * wavefront that is one flow sends ONE lane to the table: with every lane probing, the thousands of wavefronts that are resident
     * when the kernel starts would all find a hot flow's slot empty and swap on one word, 64 lanes each. */
    uint32_t head = lane;
    unsigned long long todo = __ballot(live);
    while (todo) {
        const uint32_t leader = (uint32_t)__builtin_ctzll(todo);
        kmp_flow_key k0;
        k0.a = (uint64_t)lane_value((uint32_t)(key.a >> 32), leader) << 32 | lane_value((uint32_t)key.a, leader);
        k0.b = (uint64_t)lane_value((uint32_t)(key.b >> 32), leader) << 32 | lane_value((uint32_t)key.b, leader);
        k0.proto = lane_value(key.proto, leader);
        const bool mine = live && kmp_flow_key_eq(key, k0);
        if (mine) head = leader;
        todo &= ~__ballot(mine);
    }
    uint32_t slot = 0u;
    if (live && head == lane) {
        slot = kmp_flow_hash(key) & mask;
        /* ends: more slots than payloads, so an empty slot or the flow's own lies ahead.  A plain load: a slot changes once, from 0 to
         * a payload of its flow, so a value that is not 0 is the slot's last word, and a stale 0 is put right by the swap's answer */
        for (;;) {
            uint32_t v = table[slot];
            if (v == 0u) {
                v = atomicCAS(table + slot, 0u, (uint32_t)k + 1u);
                if (v == 0u) break;
            }
            const uint4 O = meta[v - 1u];            /* (the metadata does not change: a plain load) */
            if (kmp_flow_key_eq(key, kmp_flow_key_of(O.x, O.y, O.z, O.w, directed != 0u))) break;
            slot = (slot + 1u) & mask;
        }
        /* first[slot] = min over the flow's payloads: the head is the lowest lane of its group and holds its lowest k */
        atomicMin(first + slot, (uint32_t)k);
    }
    slot = (uint32_t)__shfl((int)slot, (int)head);
    if (live) slot_of[k] = slot;
}

__global__ void __launch_bounds__(FLOW_THREADS)
kmp_flows_firsts_kernel(const uint32_t *__restrict__ first, const uint32_t *__restrict__ slot_of, uint64_t n_pkts,
                        uint32_t *__restrict__ first_len)
{
    const uint64_t k = (uint64_t)blockIdx.x * FLOW_THREADS + threadIdx.x;
    if (k < n_pkts) first_len[k] = first[slot_of[k]] == (uint32_t)k ? 16u : 0xFFFFFFFFu;
}

__global__ void __launch_bounds__(FLOW_THREADS)
kmp_flows_number_kernel(const uint4 *__restrict__ meta, uint64_t n_pkts, const uint32_t *__restrict__ first_len,
                        const uint32_t *__restrict__ loc_idx, const uint32_t *__restrict__ blk_cnt, const uint32_t *__restrict__ slot_of,
                        uint32_t *__restrict__ table, uint4 *__restrict__ recs)
{
    const uint64_t k = (uint64_t)blockIdx.x * FLOW_THREADS + threadIdx.x;
    if (k >= n_pkts || first_len[k] == 0xFFFFFFFFu) return;
    const uint32_t id = blk_cnt[k / KMP_SCAN_TILE] + loc_idx[k];
    table[slot_of[k]] = id;                          /* the slot now names the flow, no longer a payload */
    uint4 *r = recs + (uint64_t)id * (FLOW_REC_WORDS / 2u);
    r[0] = make_uint4((uint32_t)k, 0u, 0u, 0u);      /* first_packet (k < 2^32), last_packet = 0 for the maximum to come */
    r[1] = make_uint4(0u, 0u, 0u, 0u);               /* n_packets, payload_bytes */
    r[2] = meta[k];
}

__global__ void __launch_bounds__(FLOW_THREADS)
kmp_flows_assign_kernel(const uint32_t *__restrict__ table, uint32_t *__restrict__ slot_flow, const uint32_t *__restrict__ pkt_len,
                        uint64_t n_pkts, unsigned long long *__restrict__ recs)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t k = (uint64_t)blockIdx.x * FLOW_THREADS + threadIdx.x;
    const bool live = k < n_pkts;
    uint32_t f = 0u, L = 0u;
    if (live) {
        f = table[slot_flow[k]];
        slot_flow[k] = f;                            /* slot_of[k] becomes flow_of[k]: every lane reads and writes its own element */
        L = pkt_len[k];
    }
    unsigned long long todo = __ballot(live);
    while (todo) {
        const uint32_t leader = (uint32_t)__builtin_ctzll(todo);
        const uint32_t f0 = lane_value(f, leader);
        const bool mine = live && f == f0;
        const unsigned long long same = __ballot(mine);
        const uint32_t cnt = (uint32_t)__builtin_popcountll(same);
        uint64_t bytes = L;
        if (cnt > 1u) bytes = wave_sum64(mine ? (uint64_t)L : 0ull);          /* (cnt is the same in every lane) */
        if (lane == leader) {
            unsigned long long *r = recs + (uint64_t)f0 * FLOW_REC_WORDS;
            const uint64_t last = k - lane + (63u - (uint32_t)__builtin_clzll(same));
            atomicMax(r + 1, (unsigned long long)last);
            atomicAdd(r + 2, (unsigned long long)cnt);
            atomicAdd(r + 3, (unsigned long long)bytes);
        }
        todo &= ~same;
    }
}

/* A wavefront owns column word j of the payload-space rows and keeps its 64 payloads' flows in registers while the block walks the rows
 * (gridDim.y shares them out).  Per row: the word (the same address in every lane), nothing more where it is 0; the lanes whose bit is set
 * group by target word flow_of >> 6, a group ORs its bits together and its first lane issues the one atomic OR.  A group that is one flow
 * -- the whole wavefront, in a capture of big flows -- knows its bit without a cross-lane step. */
__global__ void __launch_bounds__(FLOW_THREADS)
kmp_flows_fold_kernel(const unsigned long long *__restrict__ rows, uint64_t stride, uint32_t n_rows, uint64_t n_pkts,
                      const unsigned long long *__restrict__ any, const uint32_t *__restrict__ flow_of, unsigned long long *out,
                      uint64_t stride_f)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t j = (uint64_t)blockIdx.x * FLOW_WAVES + wave;
    if (j >= (n_pkts + 63u) / 64u) return;
    if (any != nullptr && any[j] == 0ull) return;        /* no row of the family has a bit in this word */
    const uint64_t k = j * 64u + lane;
    const bool live = k < n_pkts;
    const uint32_t f = live ? flow_of[k] : 0u;
    const uint32_t tw = f >> 6;
    const unsigned long long bit = 1ull << (f & 63u);
    for (uint32_t r = blockIdx.y; r < n_rows; r += gridDim.y) {
        const unsigned long long w = rows[(uint64_t)r * stride + j];
        if (w == 0ull) continue;
        const bool on = live && ((w >> lane) & 1ull) != 0ull;
        unsigned long long todo = __ballot(on);
        while (todo) {
            const uint32_t leader = (uint32_t)__builtin_ctzll(todo);
            const uint32_t t0 = lane_value(tw, leader), f0 = lane_value(f, leader);
            const bool mine = on && tw == t0;
            const unsigned long long same = __ballot(mine), one = __ballot(on && f == f0);
            unsigned long long v = 1ull << (f0 & 63u);
            if (one != same) v = wave_or64(mine ? bit : 0ull);               /* (the same in every lane) */
            if (lane == leader) atomicOr(out + (uint64_t)r * stride_f + t0, v);
            todo &= ~same;
        }
    }
}

/* 8-byte stores from lane 0: the result is n_pkts / 8 bytes (128 KB for a million payloads) against 4 bytes of flow_of read per payload,
 * one store per 256 bytes read; a 16-byte write-out through LDS as in kmp_headers.hip would save nothing that can be seen here. */
__global__ void __launch_bounds__(FLOW_THREADS)
kmp_flows_expand_kernel(const unsigned long long *__restrict__ flow_bits, const uint32_t *__restrict__ flow_of, uint64_t n_pkts,
                        unsigned long long *__restrict__ pkt_bits)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t k = (uint64_t)blockIdx.x * FLOW_THREADS + threadIdx.x;
    bool b = false;
    if (k < n_pkts) {
        const uint32_t f = flow_of[k];
        b = ((flow_bits[f >> 6] >> (f & 63u)) & 1ull) != 0ull;
    }
    const unsigned long long w = __ballot(b);
    if (lane == 0u && k < n_pkts) pkt_bits[k >> 6] = w;
}

/* one thread per payload, no grid stride: at most 2^32 - 2 payloads are 2^24 blocks */
bool flow_grid(uint64_t n_pkts, uint32_t *blocks)
{
    if (n_pkts > 0xFFFFFFFEull) return false;
    *blocks = (uint32_t)((n_pkts + FLOW_THREADS - 1u) / FLOW_THREADS);
    return true;
}

}  // namespace

hipError_t kmp_launch_flows_insert(const void *meta, uint64_t n_pkts, bool directed, uint32_t *table, uint64_t slots, uint32_t *first,
                                   uint32_t *slot_of, hipStream_t st)
{
    static_assert(sizeof(kmpgpu_pkt_meta) == sizeof(uint4), "a metadata record is one 16-byte load");
    static_assert(sizeof(kmpgpu_flow) == FLOW_REC_WORDS * 8u, "a flow record is six 64-bit words");
    uint32_t blocks;
    if (n_pkts == 0) return hipSuccess;
    if (!flow_grid(n_pkts, &blocks) || (slots & (slots - 1u)) || slots <= n_pkts || slots > (1ull << 32)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kmp_flows_insert_kernel, dim3(blocks), dim3(FLOW_THREADS), 0, st, reinterpret_cast<const uint4 *>(meta), n_pkts,
                       directed ? 1u : 0u, table, (uint32_t)(slots - 1u), first, slot_of);
    return hipGetLastError();
}

hipError_t kmp_launch_flows_firsts(const uint32_t *first, const uint32_t *slot_of, uint64_t n_pkts, uint8_t *ws, hipStream_t st)
{
    uint32_t blocks;
    if (n_pkts == 0) return hipSuccess;
    if (!flow_grid(n_pkts, &blocks)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kmp_flows_firsts_kernel, dim3(blocks), dim3(FLOW_THREADS), 0, st, first, slot_of, n_pkts, kmp_compact_ws(ws, n_pkts).len);
    return hipGetLastError();
}

hipError_t kmp_launch_flows_number(const void *meta, uint64_t n_pkts, uint8_t *ws, const uint32_t *slot_of, uint32_t *table, void *recs,
                                   hipStream_t st)
{
    uint32_t blocks;
    if (n_pkts == 0) return hipSuccess;
    if (!flow_grid(n_pkts, &blocks)) return hipErrorInvalidValue;
    const kmp_compact_view w = kmp_compact_ws(ws, n_pkts);
    hipLaunchKernelGGL(kmp_flows_number_kernel, dim3(blocks), dim3(FLOW_THREADS), 0, st, reinterpret_cast<const uint4 *>(meta), n_pkts,
                       w.len, w.loc_idx, w.blk_cnt, slot_of, table, reinterpret_cast<uint4 *>(recs));
    return hipGetLastError();
}

hipError_t kmp_launch_flows_assign(const uint32_t *table, uint32_t *slot_flow, const uint32_t *pkt_len, uint64_t n_pkts, void *recs,
                                   hipStream_t st)
{
    uint32_t blocks;
    if (n_pkts == 0) return hipSuccess;
    if (!flow_grid(n_pkts, &blocks)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kmp_flows_assign_kernel, dim3(blocks), dim3(FLOW_THREADS), 0, st, table, slot_flow, pkt_len, n_pkts,
                       reinterpret_cast<unsigned long long *>(recs));
    return hipGetLastError();
}

hipError_t kmp_launch_flows_fold(const unsigned long long *rows, uint64_t stride, uint32_t n_rows, uint64_t n_pkts,
                                 const unsigned long long *any, const uint32_t *flow_of, uint64_t n_flows, unsigned long long *out,
                                 uint64_t stride_f, hipStream_t st)
{
    if (n_rows == 0 || n_pkts == 0) return hipSuccess;
    const uint64_t W = (n_pkts + 63u) / 64u;
    if (W > stride || (n_flows + 63u) / 64u > stride_f || n_flows == 0) return hipErrorInvalidValue;
    const uint64_t bx = (W + FLOW_WAVES - 1u) / FLOW_WAVES;
    if (bx > 0x7FFFFFFFull) return hipErrorInvalidValue;
    /* a capture too small to fill the chip with blocks of 256 payloads spreads the rows over gridDim.y (kmp_headers.hip) */
    const uint32_t by = (uint32_t)std::min<uint64_t>(std::min(n_rows, FLOW_FOLD_MAX_BY), std::max<uint64_t>(1u, 1024u / bx));
    hipLaunchKernelGGL(kmp_flows_fold_kernel, dim3((uint32_t)bx, by), dim3(FLOW_THREADS), 0, st, rows, stride, n_rows, n_pkts, any, flow_of, out,
                       stride_f);
    return hipGetLastError();
}

hipError_t kmp_launch_flows_expand(const unsigned long long *flow_bits, const uint32_t *flow_of, uint64_t n_pkts, unsigned long long *pkt_bits,
                                   hipStream_t st)
{
    uint32_t blocks;
    if (n_pkts == 0) return hipSuccess;
    if (!flow_grid(n_pkts, &blocks)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kmp_flows_expand_kernel, dim3(blocks), dim3(FLOW_THREADS), 0, st, flow_bits, flow_of, n_pkts, pkt_bits);
    return hipGetLastError();
}
