/*
 * kmp_scan_stream.hip -- the hot path on gfx950 (MI355X / CDNA4): per-pattern match counts over a
 * payload arena.  Replaces the reference loop serial.c:153-155 (= openmp_data.c:157-175) and its
 * kernel function kmp_matcher (serial.c:190-215).  Hand-written for 64-lane wavefronts; no MFMA
 * (byte scan, HBM-bound).
 *
 * Shape of the streaming kernels (flat: uniform stride, packed: any lengths)
 *   - every wavefront owns ONE contiguous byte range of the arena (whole packets) and streams it in 1 KiB chunks: one
 *     buffer_load_dwordx4 per lane (16 B), perfectly coalesced, DEPTH chunk loads in flight per wavefront in a register
 *     ring driven by hand-counted s_waitcnt vmcnt(N) (kmp_dev_common.h: ring_wait / flat_issue); the buffer resource's
 *     record count makes the tail chunk read zeros, so there is no clamping and no lane mask;
 *   - the ranges are SMALL and the grid is not persistent: ~6 KiB per wavefront for the flat kernel (four 1500-byte
 *     packets), ~16 KiB for the packed one, one block per four ranges, handed out in arena order by the hardware as CUs
 *     free up -- the whole chip reads one compact moving window of the arena (kmpgpu.hip grid_blocks,
 *     profiles/r02_flat_grid.txt: 0.89 of the HBM peak against 0.82 with one long resident range per wavefront);
 *   - still one packet per wavefront at a time: the packets of a range are scanned in order by the same
 *     wavefront, which keeps the strlen() rule (serial.c:191) wave-local state;
 *   - per chunk, every lane tests its 16 start offsets against the pattern's first dword with four v_mqsad_pk_u16_u8
 *     (masked quad byte-SAD: four offsets per instruction, byte alignment included; halo dword from the next lane by
 *     DPP wave_shl:1) and looks for 0x00 bytes with the has-zero trick; three ballots (zero lanes, packet-start lanes,
 *     candidate lanes); the common case -- no candidate in the chunk -- ends there;
 *   - rare path (confirm_sad, kmp_dev_common.h): every start offset of every candidate lane is compared in full,
 *     branch-free, by accumulating the pattern's further dwords into the filter's sums (16 bytes per block, further
 *     blocks by scalar loads); per lane the largest start index that still counts (window inside the payload, no 0x00
 *     before it) bars the rest.  The literal KMP automaton (kmp_matcher, serial.c:190-215) lives in kmp_scan_general.hip;
 *   - a start offset s counts iff s + m <= E, E = min(len, first 0x00);
 *   - counts: per-lane -> wave -> block, one partial per (block, pattern), summed by kmp_reduce_kernel
 *     (plain stores, deterministic).
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "kmp_device.h"
#include "kmp_launch.h"
#include "kmp_dev_common.h"

namespace {

/* ================================================================================================
 * Packed arenas of arbitrary payload lengths (real captures, mixed-length traffic): the same flat
 * streaming as above, with the two things the uniform kernel gets from arithmetic taken from small
 * side tables built once when the arena is loaded:
 *   - bitmap: one bit per 16-byte slot of the arena, set where a payload starts (0.8 % of the arena
 *     size); the 64 bits of a chunk ARE the packet-start ballot, fetched by one scalar load per chunk;
 *   - plan: per wavefront the first packet index and byte offset of its range.  Ranges are cut at
 *     packet starts at equal BYTE distance, which is the load balancing for mixed lengths
 *     (BASELINE configs[4]): every wavefront streams the same number of bytes whatever the lengths.
 * Lanes learn their packet (index, offset, length) only on the rare path, from the start ballot:
 * packet index = packets started before this chunk + starts at lanes <= own lane.
 * ============================================================================================== */

__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_build_bitmap_kernel(const uint64_t *__restrict__ pkt_off, uint64_t n, unsigned long long *__restrict__ bitmap)
{
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t slot = pkt_off[k] >> 4;
        atomicOr(bitmap + (slot >> 6), 1ull << (slot & 63ull));
    }
}

/* plan[w] = the packet whose start lies CLOSEST to off[0] + w * bytes_per_wave (w = 0..nwaves); plan[nwaves] = {n, end}.
 * Ranges are whole packets, so a range's length differs from bytes_per_wave by where packets happen to start; with the first start
 * at or behind the target (round 2) that was up to one packet at either end -- 9000 bytes on ~41 KB ranges for the Zipf lengths of
 * BASELINE configs[4], and a block is as slow as its slowest wavefront --, with the closest one it is half of that. */
__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_plan_kernel(const uint64_t *__restrict__ pkt_off, const uint32_t *__restrict__ pkt_len, uint64_t n, uint64_t nwaves,
                kmp_plan_shape shape, kmp_plan_entry *__restrict__ plan)
{
    const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w > nwaves) return;
    const uint64_t l16 = ((uint64_t)pkt_len[n - 1] + 15ull) & ~15ull;
    const uint64_t end = pkt_off[n - 1] + (l16 < 16ull ? 16ull : l16);
    if (w == nwaves) { plan[w].k = n; plan[w].off = end; return; }
    uint64_t target = pkt_off[0];
    if (shape.units == 0u) target += w * shape.step;
    else {
        /* unit u of region r (kmp_launch.h): the big units first, then the small ones; what a region's units overshoot belongs to the next region */
        const uint64_t r = w / shape.units, u = w % shape.units;
        const uint64_t in = u <= shape.big_units ? u * shape.step : shape.big_units * shape.step + (u - shape.big_units) * shape.small;
        target += r * shape.region + (in < shape.region ? in : shape.region);
    }
    uint64_t lo = 0, hi = n;                       /* lower_bound over the (increasing) offsets */
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (pkt_off[mid] < target) lo = mid + 1; else hi = mid;
    }
    if (lo > 0 && w > 0) {
        const uint64_t next = (lo < n) ? pkt_off[lo] : end;
        /* (a target behind the arena's end -- more wavefronts than bytes_per_wave-sized pieces -- keeps lo = n: an empty range) */
        if (next >= target && target - pkt_off[lo - 1] < next - target) --lo;      /* the start before the target is the closer one */
    }
    plan[w].k = lo;
    plan[w].off = (lo < n) ? pkt_off[lo] : end;
}

/* The flat and the packed streaming kernel: kmp_scan_stream_kernels.inc, once for the reference's strlen() rule and once for whole
 * payloads (KMPGPU_OPT_WHOLE_PAYLOAD). */
#define KMP_WHOLE false
#define KMP_FLAT_KERNEL kmp_scan_flat_kernel
#define KMP_PACKED_KERNEL kmp_scan_packed_kernel
#include "kmp_scan_stream_kernels.inc"
#undef KMP_WHOLE
#undef KMP_FLAT_KERNEL
#undef KMP_PACKED_KERNEL
#define KMP_WHOLE true
#define KMP_FLAT_KERNEL kmp_scan_flat_whole_kernel
#define KMP_PACKED_KERNEL kmp_scan_packed_whole_kernel
#include "kmp_scan_stream_kernels.inc"
#undef KMP_WHOLE
#undef KMP_FLAT_KERNEL
#undef KMP_PACKED_KERNEL

}  // namespace

namespace {
Emitter emitter_of(const kmp_scan_args &a)
{
    Emitter e{};
    e.out = reinterpret_cast<uint4 *>(a.emit_out);
    e.counter = a.emit_counter;
    e.cap = a.emit_cap;
    e.pattern = 0;
    e.marks = a.emit_marks;
    e.mark_stride = a.mark_stride;
    e.mark_rows = a.mark_rows;
    e.windows = reinterpret_cast<const uint2 *>(a.emit_windows);
    e.win_first = 0u;
    e.win_last = 0xFFFFFFFFu;
    return e;
}

template <int DEPTH>
hipError_t launch_flat_t(const kmp_scan_args &a, hipStream_t st)
{
    dim3 grid(a.blocks_x, a.n_ids), block(KMP_BLOCK_THREADS);
    const Emitter em = emitter_of(a);
#define KMP_FLAT_ARGS a.arena, a.n_pkts, a.uniform_stride, a.uniform_len, a.pkts_per_wave, a.patterns, a.pat_ids, a.partials, a.zero_counts, em
    if (a.whole) {
        /* whole payloads: four chunks in flight, the depth the dispatch takes by itself, whatever KMPGPU_OPT_DEPTH says */
        if (kmp_emits(a))
            hipLaunchKernelGGL((kmp_scan_flat_whole_kernel<4, true, true>), grid, block, 0, st, KMP_FLAT_ARGS);
        else if (a.nontemporal)
            hipLaunchKernelGGL((kmp_scan_flat_whole_kernel<4, true>), grid, block, 0, st, KMP_FLAT_ARGS);
        else
            hipLaunchKernelGGL((kmp_scan_flat_whole_kernel<4, false>), grid, block, 0, st, KMP_FLAT_ARGS);
    } else if (kmp_emits(a))
        hipLaunchKernelGGL((kmp_scan_flat_kernel<4, true, true>), grid, block, 0, st, KMP_FLAT_ARGS);
    else if (a.nontemporal)
        hipLaunchKernelGGL((kmp_scan_flat_kernel<DEPTH, true>), grid, block, 0, st, KMP_FLAT_ARGS);
    else
        hipLaunchKernelGGL((kmp_scan_flat_kernel<DEPTH, false>), grid, block, 0, st, KMP_FLAT_ARGS);
#undef KMP_FLAT_ARGS
    return hipGetLastError();
}
}  // namespace

namespace {
template <int DEPTH>
hipError_t launch_packed_t(const kmp_scan_args &a, hipStream_t st)
{
    dim3 grid(a.blocks_x, a.n_ids), block(KMP_BLOCK_THREADS);
    const kmp_plan_entry *plan = reinterpret_cast<const kmp_plan_entry *>(a.plan);
    const Emitter em = emitter_of(a);
#define KMP_PACKED_ARGS a.arena, a.pkt_off, a.pkt_len, a.bitmap, plan, a.patterns, a.pat_ids, a.partials, a.zero_counts, em, (a.pad_clean ? 1u : 0u)
    if (a.whole) {
        /* (as the flat launcher) */
        if (kmp_emits(a))
            hipLaunchKernelGGL((kmp_scan_packed_whole_kernel<4, true, true>), grid, block, 0, st, KMP_PACKED_ARGS);
        else if (a.nontemporal)
            hipLaunchKernelGGL((kmp_scan_packed_whole_kernel<4, true>), grid, block, 0, st, KMP_PACKED_ARGS);
        else
            hipLaunchKernelGGL((kmp_scan_packed_whole_kernel<4, false>), grid, block, 0, st, KMP_PACKED_ARGS);
    } else if (kmp_emits(a))
        hipLaunchKernelGGL((kmp_scan_packed_kernel<4, true, true>), grid, block, 0, st, KMP_PACKED_ARGS);
    else if (a.nontemporal)
        hipLaunchKernelGGL((kmp_scan_packed_kernel<DEPTH, true>), grid, block, 0, st, KMP_PACKED_ARGS);
    else
        hipLaunchKernelGGL((kmp_scan_packed_kernel<DEPTH, false>), grid, block, 0, st, KMP_PACKED_ARGS);
#undef KMP_PACKED_ARGS
    return hipGetLastError();
}
}  // namespace

/* Flat streaming kernel for packed arenas of arbitrary payload lengths (bitmap + plan from kmp_launch_prepare_packed). */
hipError_t kmp_launch_scan_packed(const kmp_scan_args &a, hipStream_t st)
{
    if (a.n_ids == 0 || a.blocks_x == 0) return hipSuccess;
    switch (a.depth) {          /* 0 = auto: 4 chunks in flight with the 16 KiB ranges (profiles/r02_flat_grid.txt; 3 with the persistent grid of round 1) */
    case 2: case 3: return launch_packed_t<3>(a, st);
    case 6: case 8: return launch_packed_t<6>(a, st);
    default: return launch_packed_t<4>(a, st);
    }
}

hipError_t kmp_launch_build_bitmap(const uint64_t *pkt_off, uint64_t n, unsigned long long *bitmap, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    uint64_t blocks = (n + KMP_BLOCK_THREADS - 1) / KMP_BLOCK_THREADS;
    if (blocks > 4096u) blocks = 4096u;
    hipLaunchKernelGGL(kmp_build_bitmap_kernel, dim3((uint32_t)blocks), dim3(KMP_BLOCK_THREADS), 0, st, pkt_off, n, bitmap);
    return hipGetLastError();
}

hipError_t kmp_launch_plan(const uint64_t *pkt_off, const uint32_t *pkt_len, uint64_t n, uint64_t nwaves, const kmp_plan_shape &shape,
                           void *plan, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    const uint64_t blocks = (nwaves + 1 + KMP_BLOCK_THREADS - 1) / KMP_BLOCK_THREADS;
    hipLaunchKernelGGL(kmp_plan_kernel, dim3((uint32_t)blocks), dim3(KMP_BLOCK_THREADS), 0, st, pkt_off, pkt_len, n, nwaves,
                       shape, reinterpret_cast<kmp_plan_entry *>(plan));
    return hipGetLastError();
}

/* Flat streaming kernel for uniform-stride arenas (a.arena already points at payload 0). */
hipError_t kmp_launch_scan_flat(const kmp_scan_args &a, hipStream_t st)
{
    if (a.n_ids == 0 || a.blocks_x == 0) return hipSuccess;
    switch (a.depth) {
    case 2: return launch_flat_t<2>(a, st);
    case 3: return launch_flat_t<3>(a, st);
    case 5: return launch_flat_t<5>(a, st);
    case 6: return launch_flat_t<6>(a, st);
    case 8: return launch_flat_t<8>(a, st);
    default: return launch_flat_t<4>(a, st);
    }
}

