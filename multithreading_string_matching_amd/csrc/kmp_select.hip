/*
 * kmp_select.hip -- kmpgpu_load_selected: the payloads a bitmap selects, compacted on the device into a packed arena (kmpgpu.h).  gfx950.
 *
 *   kmp_select_lengths_kernel   sel_len[k] = bit k of the bitmap ? len[k] : 0xFFFFFFFF ("rejected", as kmp_extract_kernel writes it); a
 *                               wavefront's 64 payloads share one bitmap word, bits at n and above are never looked at
 *   kmp_scan_local_kernel, kmp_scan_totals_kernel   of kmp_prep.hip, through kmp_launch_repack_phase1: slot offsets and payload
 *                               numbers of the selected payloads, totals = {packed bytes, payloads}
 *   kmp_select_index_kernel     the new index, and per selected payload the record {source offset, length} the copy reads
 *   kmp_select_copy_kernel      the bytes
 *
 * The copy.  Source slots and destination slots are 16-byte aligned, so a payload moves in 16-byte units, and the destination is packed:
 * the units of consecutive payloads are consecutive.  A wavefront takes a RUN of up to 64 consecutive selected payloads.  Their new
 * offsets ARE the prefix sums of their unit counts (kmp_select_index_kernel has just written them), so nothing is summed here: lane i
 * puts offset, source and length of payload i of the run into the wavefront's 1.25 KiB of LDS, and the run's units are then dealt out
 * to the lanes in order, 64 consecutive units per step -- one contiguous KiB of stores whatever the payload boundaries.  A lane finds
 * the payload of its unit with a branch-free binary search over the run's offsets (6 LDS reads), reads the unit from the source, clears
 * in registers what lies behind the payload's end, and stores it.  KMP_SELECT_UNROLL units per lane are in flight before the first
 * store.  64-byte payloads keep every lane busy (a run is 4 KiB), where one wavefront per payload (kmp_gather_kernel) idles 60 of 64;
 * 1500-byte payloads get runs of 8 (12 KiB).  The other shape -- a fixed byte range of the destination per wavefront, found by a
 * binary search in the new offsets -- balances bytes exactly but walks the index with data-dependent global loads per range; runs of
 * payloads read the index once, coalesced, and the run length evens the bytes out well enough (kmp_launch_select_phase2).
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "kmp_device.h"
#include "kmp_launch.h"

namespace {

typedef uint32_t sel_u32x4 __attribute__((ext_vector_type(4)));

constexpr uint32_t KMP_SELECT_UNROLL = 4;            /* 16-byte units a lane has in flight */
constexpr uint32_t KMP_SELECT_INDEX_BLOCKS = 1024;   /* grid cap of the two index kernels: rounds past 262 144 payloads */
constexpr uint32_t KMP_SELECT_COPY_BLOCKS = 1024;    /* grid cap of the copy kernel (16 wavefronts per CU): rounds past 4 096 runs */
constexpr uint32_t KMP_SELECT_RUN_BYTES = 16384;     /* bytes a run should come to */

/* The scan workspace of kmp_prep.hip (kmp_extract_ws_bytes): loc_off[n], blk_bytes[nblk], then the 32-bit arrays poff[n], plen[n],
 * loc_idx[n], blk_cnt[nblk].  The masked lengths take plen's place; poff is not used. */
struct SelectWs {
    uint64_t *loc_off, *blk_bytes;
    uint32_t *sel_len, *loc_idx, *blk_cnt;
};
SelectWs select_ws(uint8_t *ws, uint64_t n)
{
    const uint64_t nblk = (n + KMP_SCAN_TILE - 1) / KMP_SCAN_TILE;
    SelectWs w;
    w.loc_off = reinterpret_cast<uint64_t *>(ws);
    w.blk_bytes = w.loc_off + n;
    w.sel_len = reinterpret_cast<uint32_t *>(w.blk_bytes + nblk) + n;
    w.loc_idx = w.sel_len + n;
    w.blk_cnt = w.loc_idx + n;
    return w;
}

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
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t l = sel_len[k];
        if (l == 0xFFFFFFFFu) continue;
        const uint64_t blk = k / KMP_SCAN_TILE;
        const uint64_t j = (uint64_t)blk_cnt[blk] + loc_idx[k];
        const uint64_t so = src_off[k];
        pkt_off[j] = blk_bytes[blk] + loc_off[k];
        pkt_len[j] = l;
        recs[j] = make_uint4((uint32_t)so, (uint32_t)(so >> 32), l, 0u);
    }
}

template <bool NT>
__device__ __forceinline__ sel_u32x4 load_unit(const uint8_t *p)
{
    const sel_u32x4 *q = reinterpret_cast<const sel_u32x4 *>(p);
    return NT ? __builtin_nontemporal_load(q) : *q;
}
template <bool NT>
__device__ __forceinline__ void store_unit(uint8_t *p, sel_u32x4 v)
{
    sel_u32x4 *q = reinterpret_cast<sel_u32x4 *>(p);
    if (NT) __builtin_nontemporal_store(v, q); else *q = v;
}

/* the bytes [keep, 16) of a unit cleared; keep >= 16 leaves it whole */
__device__ __forceinline__ sel_u32x4 keep_bytes(sel_u32x4 v, uint32_t keep)
{
    uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (uint32_t d = 0; d < 4u; ++d) {
        const uint32_t lo = 4u * d;
        w[d] &= (keep >= lo + 4u) ? 0xFFFFFFFFu : (keep <= lo) ? 0u : ((1u << (8u * (keep - lo))) - 1u);
    }
    sel_u32x4 r; r.x = w[0]; r.y = w[1]; r.z = w[2]; r.w = w[3];
    return r;
}

template <bool NT>
__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_select_copy_kernel(const uint8_t *__restrict__ src, const uint64_t *__restrict__ new_off, const uint4 *__restrict__ recs, uint64_t n,
                       uint64_t total, uint32_t run, uint8_t *__restrict__ dst)
{
    __shared__ uint64_t s_off[KMP_BLOCK_WAVES][KMP_WAVE];          /* new offset of payload i of the run; ~0 behind the run's end */
    __shared__ uint64_t s_src[KMP_BLOCK_WAVES][KMP_WAVE];
    __shared__ uint32_t s_len[KMP_BLOCK_WAVES][KMP_WAVE];
    const uint32_t lane = threadIdx.x & (KMP_WAVE - 1u), wid = threadIdx.x >> 6;
    const uint64_t n_runs = (n + run - 1u) / run;
    for (uint64_t r = (uint64_t)blockIdx.x * KMP_BLOCK_WAVES + wid; r < n_runs; r += (uint64_t)gridDim.x * KMP_BLOCK_WAVES) {
        const uint64_t j0 = r * run, j = j0 + lane;
        uint64_t off = ~0ull, so = 0ull;
        uint32_t len = 0u;
        if (lane < run && j < n) {
            const uint4 rec = recs[j];
            off = new_off[j];
            so = ((uint64_t)rec.y << 32) | rec.x;
            len = rec.z;
        }
        /* the wavefront's own LDS: its DS instructions execute in order, the barriers keep the compiler from moving them */
        __builtin_amdgcn_wave_barrier();
        s_off[wid][lane] = off; s_src[wid][lane] = so; s_len[wid][lane] = len;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const uint64_t base = new_off[j0];
        const uint64_t end = (j0 + run < n) ? new_off[j0 + run] : total;
        for (uint64_t d0 = base + (uint64_t)lane * 16u; d0 - lane * 16u < end; d0 += (uint64_t)KMP_SELECT_UNROLL * KMP_WAVE * 16u) {
            sel_u32x4 v[KMP_SELECT_UNROLL];
            uint32_t keep[KMP_SELECT_UNROLL];
#pragma unroll
            for (uint32_t u = 0; u < KMP_SELECT_UNROLL; ++u) {
                const uint64_t d = d0 + (uint64_t)u * KMP_WAVE * 16u;
                v[u] = (sel_u32x4)(0u);
                keep[u] = 0u;
                if (d < end) {
                    uint32_t p = 0u;                                 /* the last payload of the run that starts at or before d */
#pragma unroll
                    for (uint32_t step = KMP_WAVE / 2u; step; step >>= 1)
                        if (s_off[wid][p + step] <= d) p += step;
                    const uint64_t rel = d - s_off[wid][p];
                    const uint32_t L = s_len[wid][p];
                    if (rel < L) {                                   /* (an empty payload's slot, or nothing: zeros) */
                        v[u] = load_unit<NT>(src + s_src[wid][p] + rel);
                        keep[u] = (uint32_t)min((uint64_t)16u, (uint64_t)L - rel);
                    }
                }
            }
#pragma unroll
            for (uint32_t u = 0; u < KMP_SELECT_UNROLL; ++u) {
                const uint64_t d = d0 + (uint64_t)u * KMP_WAVE * 16u;
                if (d < end) store_unit<NT>(dst + d, keep_bytes(v[u], keep[u]));
            }
        }
    }
}

}  // namespace

/* Phase 1: masked lengths + scan; totals[0] = bytes of the packed selection, totals[1] = selected payloads.  ws:
 * kmp_extract_ws_bytes(n) bytes, kept until phase 2. */
hipError_t kmp_launch_select_phase1(const unsigned long long *select, const uint32_t *pkt_len, uint64_t n, uint8_t *ws,
                                    unsigned long long *totals, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    const SelectWs w = select_ws(ws, n);
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((n + KMP_BLOCK_THREADS - 1) / KMP_BLOCK_THREADS, KMP_SELECT_INDEX_BLOCKS);
    hipLaunchKernelGGL(kmp_select_lengths_kernel, dim3(blocks), dim3(KMP_BLOCK_THREADS), 0, st, select, pkt_len, n, w.sel_len);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return kmp_launch_repack_phase1(w.sel_len, n, ws, totals, st);          /* kmp_scan_local_kernel + kmp_scan_totals_kernel */
}

/* Phase 2: index of the selection (pkt_off, pkt_len: n_sel entries; recs: n_sel 16-byte records) and the copy of its total_bytes. */
hipError_t kmp_launch_select_phase2(const uint8_t *src_arena, const uint64_t *src_off, uint64_t n, uint8_t *ws, uint64_t n_sel,
                                    uint64_t total_bytes, uint8_t *arena, uint64_t *pkt_off, uint32_t *pkt_len, void *recs,
                                    bool nontemporal, hipStream_t st)
{
    if (n == 0 || n_sel == 0) return hipSuccess;
    const SelectWs w = select_ws(ws, n);
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((n + KMP_BLOCK_THREADS - 1) / KMP_BLOCK_THREADS, KMP_SELECT_INDEX_BLOCKS);
    hipLaunchKernelGGL(kmp_select_index_kernel, dim3(blocks), dim3(KMP_BLOCK_THREADS), 0, st, src_off, w.sel_len, w.loc_off, w.loc_idx,
                       w.blk_bytes, w.blk_cnt, n, pkt_off, pkt_len, (uint4 *)recs);
    /* payloads per run: what brings an average run to KMP_SELECT_RUN_BYTES, a power of two up to 64 */
    const uint64_t avg = std::max<uint64_t>(total_bytes / n_sel, 16);
    uint32_t run = KMP_WAVE;
    while (run > 1u && (uint64_t)run * avg > KMP_SELECT_RUN_BYTES) run >>= 1;
    const uint64_t n_runs = (n_sel + run - 1) / run;
    const uint32_t cblocks = (uint32_t)std::min<uint64_t>((n_runs + KMP_BLOCK_WAVES - 1) / KMP_BLOCK_WAVES, KMP_SELECT_COPY_BLOCKS);
    if (nontemporal)
        hipLaunchKernelGGL(kmp_select_copy_kernel<true>, dim3(cblocks), dim3(KMP_BLOCK_THREADS), 0, st, src_arena, pkt_off, (const uint4 *)recs,
                           n_sel, total_bytes, run, arena);
    else
        hipLaunchKernelGGL(kmp_select_copy_kernel<false>, dim3(cblocks), dim3(KMP_BLOCK_THREADS), 0, st, src_arena, pkt_off, (const uint4 *)recs,
                           n_sel, total_bytes, run, arena);
    return hipGetLastError();
}
