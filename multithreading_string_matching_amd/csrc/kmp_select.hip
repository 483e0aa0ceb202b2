/*
 * kmp_select.hip -- kmpgpu_load_selected: the payloads a bitmap selects, compacted on the device into a packed arena (kmpgpu.h).  gfx950.
 *
 *   kmp_select_lengths_kernel   sel_len[k] = bit k of the bitmap ? len[k] : 0xFFFFFFFF ("rejected", as kmp_extract_kernel writes it); a
 *                               wavefront's 64 payloads share one bitmap word, bits at n and above are never looked at
 *   kmp_scan_local_kernel, kmp_scan_totals_kernel   of kmp_prep.hip, through kmp_launch_compact_scan
 *   kmp_select_index_kernel     the new index, and per selected payload the record {source offset, length} the copy reads
 *   kmp_select_copy_kernel      the bytes
 *
 * The four steps and the copy's shape -- a wavefront per RUN of consecutive selected payloads, the run's 16-byte units dealt to the lanes
 * in order -- are the compacting skeleton's (kmp_compact_dev.h).  What is this file's own: source slots and destination slots
 * are both 16-byte aligned, so a destination unit is ONE aligned source unit, cleared behind the payload's end in registers at the
 * store, and four units per lane are in flight.  64-byte payloads keep every lane busy (a run is 4 KiB), where one wavefront per payload
 * (kmp_gather_kernel) idles 60 of 64; 1500-byte payloads get runs of 8 (12 KiB).
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kmp_device.h"
#include "kmp_launch.h"
#include "kmp_compact_dev.h"

namespace {

using namespace kmp_unit;     /* kmp_compact_dev.h: index_body, gather_runs; kmp_unit_dev.h: the unit */

__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_select_lengths_kernel(const unsigned long long *__restrict__ select, const uint32_t *__restrict__ pkt_len, uint64_t n,
                          uint32_t *__restrict__ sel_len)
{
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (uint64_t)gridDim.x * blockDim.x)
        sel_len[k] = ((select[k >> 6] >> (k & 63u)) & 1ull) ? pkt_len[k] : 0xFFFFFFFFu;      /* (k >> 6 is one word per wavefront) */
}

/* Payload k of the source is payload j of the selection: its slot in the new arena, its length, and where its bytes lie. */
__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_select_index_kernel(const uint64_t *__restrict__ src_off, const uint32_t *__restrict__ sel_len, const uint64_t *__restrict__ loc_off,
                        const uint32_t *__restrict__ loc_idx, const uint64_t *__restrict__ blk_bytes, const uint32_t *__restrict__ blk_cnt,
                        uint64_t n, uint64_t *__restrict__ pkt_off, uint32_t *__restrict__ pkt_len, uint4 *__restrict__ recs)
{
    index_body(sel_len, loc_off, loc_idx, blk_bytes, blk_cnt, n, pkt_off, pkt_len, recs, [&](uint64_t k, uint32_t l) {
        const uint64_t so = src_off[k];
        return make_uint4((uint32_t)so, (uint32_t)(so >> 32), l, 0u);
    });
}

template <bool NT>
__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_select_copy_kernel(const uint8_t *__restrict__ src, const uint64_t *__restrict__ new_off, const uint4 *__restrict__ recs, uint64_t n,
                       uint64_t total, uint32_t run, uint8_t *__restrict__ dst)
{
    __shared__ uint64_t s_src[KMP_BLOCK_WAVES][KMP_WAVE];
    __shared__ uint32_t s_len[KMP_BLOCK_WAVES][KMP_WAVE];
    const uint32_t lane = threadIdx.x & (KMP_WAVE - 1u), wid = threadIdx.x >> 6;
    gather_runs<NT, 4>(new_off, n, total, run, dst,
        [&](uint64_t j, bool in) { return in ? recs[j] : make_uint4(0u, 0u, 0u, 0u); },
        [&](uint4 rec) {
            s_src[wid][lane] = ((uint64_t)rec.y << 32) | rec.x; s_len[wid][lane] = rec.z;
        },
        [&](uint32_t p, uint64_t rel, uint32_t &keep) {
            const uint32_t L = s_len[wid][p];
            if (rel >= L) return (u32x4)(0u);                        /* (an empty payload's slot, or nothing: zeros) */
            keep = (uint32_t)min((uint64_t)16u, (uint64_t)L - rel);
            return load_unit<NT>(src + s_src[wid][p] + rel);         /* source slots are 16-byte aligned, as the destination's are */
        });
}

}  // namespace

/* Phase 1: masked lengths + scan; totals[0] = bytes of the packed selection, totals[1] = selected payloads.  ws:
 * kmp_extract_ws_bytes(n) bytes, kept until phase 2. */
hipError_t kmp_launch_select_phase1(const unsigned long long *select, const uint32_t *pkt_len, uint64_t n, uint8_t *ws,
                                    unsigned long long *totals, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(kmp_select_lengths_kernel, dim3(kmp_item_blocks(n)), dim3(KMP_BLOCK_THREADS), 0, st, select, pkt_len, n, kmp_compact_ws(ws, n).len);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return kmp_launch_compact_scan(n, ws, totals, st);
}

/* Phase 2: index of the selection (pkt_off, pkt_len: n_sel entries; recs: n_sel 16-byte records) and the copy of its total_bytes. */
hipError_t kmp_launch_select_phase2(const uint8_t *src_arena, const uint64_t *src_off, uint64_t n, uint8_t *ws, uint64_t n_sel,
                                    uint64_t total_bytes, uint8_t *arena, uint64_t *pkt_off, uint32_t *pkt_len, void *recs,
                                    bool nontemporal, hipStream_t st)
{
    if (n == 0 || n_sel == 0) return hipSuccess;
    const kmp_compact_view w = kmp_compact_ws(ws, n);
    hipLaunchKernelGGL(kmp_select_index_kernel, dim3(kmp_item_blocks(n)), dim3(KMP_BLOCK_THREADS), 0, st, src_off, w.len, w.loc_off, w.loc_idx,
                       w.blk_bytes, w.blk_cnt, n, pkt_off, pkt_len, (uint4 *)recs);
    const kmp_run_shape rs = kmp_run_shape_of(n_sel, total_bytes);
    hipLaunchKernelGGL(nontemporal ? kmp_select_copy_kernel<true> : kmp_select_copy_kernel<false>, dim3(rs.blocks), dim3(KMP_BLOCK_THREADS), 0, st,
                       src_arena, pkt_off, (const uint4 *)recs, n_sel, total_bytes, rs.run, arena);
    return hipGetLastError();
}
