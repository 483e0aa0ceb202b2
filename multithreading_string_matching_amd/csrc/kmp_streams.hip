/*
 * kmp_streams.hip -- kmpgpu_load_streams: the payloads of every (flow, direction) of an index whose flows are built, concatenated in
 * capture order and cut to `depth` bytes, as one payload each of a packed arena (kmpgpu.h).  gfx950.
 *
 *   kmp_seam_keys_kernel, rocprim::radix_sort_pairs   of kmp_seams.hip, as they are: (flow_of[k] << 1 | dir(k), k) sorted by key, stably
 *   kmp_stream_scan_kernel    at sorted position i: head[i] = key[i] != key[i - 1], and the tile-local exclusive sum of the members' lengths
 *                             (64 bits) and inclusive count of heads, as kmp_scan_local_kernel does for slot sizes
 *   kmp_stream_totals_kernel  the tiles' totals scanned in place; totals = {bytes of all members, n_streams}
 *   kmp_stream_heads_kernel   head_pos[s] = the sorted position stream s starts at, head_pos[n_streams] = n
 *   kmp_stream_records_kernel per stream: its kmpgpu_stream record, len = min(bytes, depth), meta[s] = src.meta[first_packet]
 *   kmp_scan_local_kernel, kmp_scan_totals_kernel   of kmp_prep.hip, through kmp_launch_repack_phase1 over len[]: the slot offsets
 *   kmp_stream_index_kernel   per stream: pkt_off, pkt_len; per sorted position: the member's kmpgpu_stream_pos entry, and its PIECE: where it
 *                             lies in the source, where it goes in the arena, how much of it is in front of the cut
 *   kmp_stream_gather_kernel  the bytes
 *
 * pos is the plain exclusive sum at i minus its value at the stream's head; no atomic decides a value anywhere.
 *
 * The gather.  The arena is written in 16-byte units, every unit of [0, total) exactly once, a wavefront's 64 lanes storing 64 consecutive
 * units.  Pieces are in sorted order, which is ascending destination address, so the piece that holds a unit's first byte is the last one
 * whose destination is not behind it: a search over piece_dst[].  The search runs over the global array, not over a table in LDS as the seam
 * gather's does, because a unit can be made of any number of pieces (sixteen 1-byte members, 0-byte ones in between), so no fixed number of
 * table entries covers a wavefront's units; instead each wavefront takes one CONTIGUOUS span of the arena and carries its place in the piece
 * array forward: one full search per wavefront, then a galloping step from the last place, which for members longer than a unit is one 8-byte
 * load that neighbouring lanes share.  From that piece the lane walks on while pieces start inside its unit.  Each piece's bytes are fetched
 * as in kmp_seams.hip: ALIGNED 16-byte loads of the source units that hold a wanted byte -- one or two --, a byte funnel shift
 * (v_alignbyte_b32), a mask in registers, and an OR.  An aligned unit that holds a byte of a member lies inside that member's slot, so no byte
 * outside the members' slots is read.  Everything behind a stream's end comes out 0x00 because no piece covers it.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "kmpgpu.h"
#include "kmp_device.h"
#include "kmp_launch.h"
#include "kmp_piece_dev.h"

namespace {

using kmp_piece::u32x4;

/* A lane's units are looked up one after the other (piece_dst -> piece record -> source units: three dependent loads each), so what
 * is in flight is one unit per lane: parallelism comes from wavefronts, 8 per SIMD (40 VGPRs allow them), not from units per lane. */
constexpr uint32_t STREAM_UNROLL = 1;             /* destination units a lane takes per round */
constexpr uint32_t STREAM_INDEX_BLOCKS = 1024;    /* grid cap of the per-payload and per-stream kernels: rounds past 262 144 elements */
constexpr uint32_t STREAM_GATHER_BLOCKS = 2048;   /* grid cap of the gather (32 wavefronts per CU) */
constexpr uint64_t STREAM_CHUNK_UNITS = (uint64_t)STREAM_UNROLL * KMP_WAVE;      /* units a wavefront writes per round: 1 KiB */

/* The sorted pairs inside the sort buffer, as kmp_seams.hip lays them out (seam_sort there): keys in / out, values in / out. */
struct StreamSorted { const uint64_t *key; const uint32_t *val; };
StreamSorted stream_sorted(const uint8_t *buf, uint64_t n)
{
    StreamSorted s;
    s.key = reinterpret_cast<const uint64_t *>(buf) + n;
    s.val = reinterpret_cast<const uint32_t *>(s.key + n) + n;
    return s;
}

/* The workspace: first what kmp_launch_repack_phase1 needs for up to n streams (its loc_off[] and blk_bytes[] are read back here), then
 * this file's own arrays over the n sorted positions. */
struct StreamWs {
    uint8_t  *scan;                                /* kmp_extract_ws_bytes(n) bytes, 256-byte rounded */
    uint64_t *sum, *blk_sum;                       /* [n] tile-local exclusive sums of the lengths, [nblk] the tiles' */
    uint32_t *head_pos, *slen, *cnt, *blk_cnt;     /* [n + 1], [n], [n] tile-local inclusive head counts, [nblk] */
};
uint64_t stream_scan_bytes(uint64_t n) { return ((uint64_t)kmp_extract_ws_bytes(n) + 255u) & ~255ull; }
StreamWs stream_ws(uint8_t *ws, uint64_t n)
{
    const uint64_t nblk = (n + KMP_SCAN_TILE - 1) / KMP_SCAN_TILE;
    StreamWs w;
    w.scan = ws;
    w.sum = reinterpret_cast<uint64_t *>(ws + stream_scan_bytes(n));
    w.blk_sum = w.sum + n;
    w.head_pos = reinterpret_cast<uint32_t *>(w.blk_sum + nblk);
    w.slen = w.head_pos + n + 1u;
    w.cnt = w.slen + n;
    w.blk_cnt = w.cnt + n;
    return w;
}

__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_stream_scan_kernel(const uint64_t *__restrict__ key, const uint32_t *__restrict__ val, const uint32_t *__restrict__ pkt_len, uint64_t n,
                       uint64_t *__restrict__ sum, uint32_t *__restrict__ cnt, uint64_t *__restrict__ blk_sum, uint32_t *__restrict__ blk_cnt)
{
    __shared__ uint64_t s_b[KMP_BLOCK_THREADS];
    __shared__ uint32_t s_c[KMP_BLOCK_THREADS];
    const uint64_t base = (uint64_t)blockIdx.x * KMP_SCAN_TILE + (uint64_t)threadIdx.x * KMP_SCAN_ITEMS;
    uint64_t b[KMP_SCAN_ITEMS], tb = 0;
    uint32_t c[KMP_SCAN_ITEMS], tc = 0;
#pragma unroll
    for (uint32_t i = 0; i < KMP_SCAN_ITEMS; i++) {
        const uint64_t j = base + i;
        uint32_t l = 0u, head = 0u;
        if (j < n) {
            l = pkt_len[val[j]];
            head = (j == 0 || key[j - 1] != key[j]) ? 1u : 0u;
        }
        tc += head;
        b[i] = tb; c[i] = tc;                                         /* exclusive sum, inclusive count */
        tb += l;
    }
    s_b[threadIdx.x] = tb; s_c[threadIdx.x] = tc;
    __syncthreads();
    for (uint32_t d = 1; d < KMP_BLOCK_THREADS; d <<= 1) {            /* Hillis-Steele inclusive scan of the thread totals */
        const uint64_t vb = threadIdx.x >= d ? s_b[threadIdx.x - d] : 0ull;
        const uint32_t vc = threadIdx.x >= d ? s_c[threadIdx.x - d] : 0u;
        __syncthreads();
        s_b[threadIdx.x] += vb; s_c[threadIdx.x] += vc;
        __syncthreads();
    }
    const uint64_t eb = s_b[threadIdx.x] - tb;
    const uint32_t ec = s_c[threadIdx.x] - tc;
#pragma unroll
    for (uint32_t i = 0; i < KMP_SCAN_ITEMS; i++)
        if (base + i < n) { sum[base + i] = eb + b[i]; cnt[base + i] = ec + c[i]; }
    if (threadIdx.x == KMP_BLOCK_THREADS - 1u) { blk_sum[blockIdx.x] = s_b[threadIdx.x]; blk_cnt[blockIdx.x] = s_c[threadIdx.x]; }
}

/* One block: exclusive scan of the tile totals in place; totals[0] = bytes of all members, totals[1] = streams. */
__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_stream_totals_kernel(uint64_t *__restrict__ blk_sum, uint32_t *__restrict__ blk_cnt, uint32_t nblk, unsigned long long *__restrict__ totals)
{
    __shared__ uint64_t s_b[KMP_BLOCK_THREADS];
    __shared__ uint32_t s_c[KMP_BLOCK_THREADS];
    uint64_t cb = 0, cc = 0;
    for (uint32_t base = 0; base < nblk; base += KMP_BLOCK_THREADS) {
        const uint32_t i = base + threadIdx.x;
        const uint64_t vb0 = i < nblk ? blk_sum[i] : 0ull;
        const uint32_t vc0 = i < nblk ? blk_cnt[i] : 0u;
        s_b[threadIdx.x] = vb0; s_c[threadIdx.x] = vc0;
        __syncthreads();
        for (uint32_t d = 1; d < KMP_BLOCK_THREADS; d <<= 1) {
            const uint64_t vb = threadIdx.x >= d ? s_b[threadIdx.x - d] : 0ull;
            const uint32_t vc = threadIdx.x >= d ? s_c[threadIdx.x - d] : 0u;
            __syncthreads();
            s_b[threadIdx.x] += vb; s_c[threadIdx.x] += vc;
            __syncthreads();
        }
        if (i < nblk) { blk_sum[i] = cb + s_b[threadIdx.x] - vb0; blk_cnt[i] = (uint32_t)(cc + s_c[threadIdx.x] - vc0); }
        cb += s_b[KMP_BLOCK_THREADS - 1u]; cc += s_c[KMP_BLOCK_THREADS - 1u];
        __syncthreads();
    }
    if (threadIdx.x == 0u) { totals[0] = cb; totals[1] = cc; }
}

__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_stream_heads_kernel(const uint64_t *__restrict__ key, const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ blk_cnt, uint64_t n,
                        uint64_t n_streams, uint32_t *__restrict__ head_pos)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        if (i == 0 || key[i - 1] != key[i]) head_pos[(uint64_t)blk_cnt[i / KMP_SCAN_TILE] + cnt[i] - 1u] = (uint32_t)i;
        if (i == n - 1u) head_pos[n_streams] = (uint32_t)n;
    }
}

/* the exclusive sum of the members' lengths at sorted position i <= n */
__device__ __forceinline__ uint64_t sum_at(const uint64_t *__restrict__ sum, const uint64_t *__restrict__ blk_sum, uint64_t i, uint64_t n,
                                           uint64_t total)
{
    return i < n ? blk_sum[i / KMP_SCAN_TILE] + sum[i] : total;
}

__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_stream_records_kernel(const uint64_t *__restrict__ key, const uint32_t *__restrict__ val, const uint4 *__restrict__ src_meta,
                          const uint64_t *__restrict__ sum, const uint64_t *__restrict__ blk_sum, const uint32_t *__restrict__ head_pos,
                          uint64_t n, uint64_t total, uint64_t n_streams, uint32_t depth, uint64_t *__restrict__ recs,
                          uint32_t *__restrict__ slen, uint4 *__restrict__ meta)
{
    for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n_streams; s += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t h = head_pos[s], e = head_pos[s + 1u];
        const uint64_t bytes = sum_at(sum, blk_sum, e, n, total) - sum_at(sum, blk_sum, h, n, total);
        const uint32_t len = (uint32_t)min(bytes, (uint64_t)depth);
        const uint64_t k = key[h];
        const uint32_t first = val[h];
        recs[6u * s] = first;                                        /* kmpgpu_stream: first_packet, last_packet, n_packets, bytes, */
        recs[6u * s + 1u] = val[e - 1u];
        recs[6u * s + 2u] = e - h;
        recs[6u * s + 3u] = bytes;
        recs[6u * s + 4u] = (k & 1u) << 32 | (k >> 1);               /* flow | dir << 32, len | 0 << 32 */
        recs[6u * s + 5u] = len;
        slen[s] = len;
        meta[s] = src_meta[first];
    }
}

/* loc_off / blk_bytes: what kmp_launch_repack_phase1 left over slen[n_streams] (loc_off[n_streams], then the tiles' offsets). */
__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_stream_index_kernel(const uint32_t *__restrict__ val, const uint64_t *__restrict__ src_off, const uint32_t *__restrict__ src_len,
                        const uint64_t *__restrict__ sum, const uint64_t *__restrict__ blk_sum, const uint32_t *__restrict__ cnt,
                        const uint32_t *__restrict__ blk_cnt, const uint32_t *__restrict__ head_pos, const uint32_t *__restrict__ slen,
                        const uint64_t *__restrict__ loc_off, const uint64_t *__restrict__ blk_bytes, uint64_t n, uint64_t total,
                        uint64_t n_streams, uint64_t *__restrict__ pkt_off, uint32_t *__restrict__ pkt_len, uint4 *__restrict__ map,
                        uint4 *__restrict__ piece, uint64_t *__restrict__ piece_dst)
{
    const uint64_t t0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t s = t0; s < n_streams; s += step) {
        pkt_off[s] = blk_bytes[s / KMP_SCAN_TILE] + loc_off[s];
        pkt_len[s] = slen[s];
    }
    for (uint64_t i = t0; i < n; i += step) {
        const uint32_t k = val[i];
        const uint64_t s = (uint64_t)blk_cnt[i / KMP_SCAN_TILE] + cnt[i] - 1u;
        const uint64_t pos = sum_at(sum, blk_sum, i, n, total) - sum_at(sum, blk_sum, head_pos[s], n, total);
        const uint32_t len = slen[s], L = src_len[k];
        /* a member at or behind the cut: no byte, at the stream's end (destinations stay ascending) */
        const uint32_t at = (uint32_t)min(pos, (uint64_t)len), take = min(L, len - at);
        const uint64_t so = src_off[k];
        map[k] = make_uint4((uint32_t)s, 0u, (uint32_t)pos, (uint32_t)(pos >> 32));      /* kmpgpu_stream_pos: stream, 0, pos */
        piece[i] = make_uint4((uint32_t)so, (uint32_t)(so >> 32), take, 0u);
        piece_dst[i] = blk_bytes[s / KMP_SCAN_TILE] + loc_off[s] + at;
    }
}

/* load_unit / store_unit / fetch_piece: kmp_piece_dev.h, which the gathers of the derived arenas share */
using kmp_piece::fetch_piece;
using kmp_piece::load_unit;
using kmp_piece::store_unit;

/* The last piece q >= p with piece_dst[q] <= d, given piece_dst[p] <= d: galloping, then halving.  One load where the next piece starts
 * behind d. */
__device__ __forceinline__ uint32_t advance_piece(const uint64_t *__restrict__ piece_dst, uint64_t n, uint32_t p, uint64_t d)
{
    uint64_t q = p, step = 1;
    while (q + step < n && piece_dst[q + step] <= d) { q += step; step <<= 1; }
    for (step >>= 1; step; step >>= 1)
        if (q + step < n && piece_dst[q + step] <= d) q += step;
    return (uint32_t)q;
}

/* Wavefront w of all W writes the units [w * span, (w + 1) * span) of the arena's `units`, span a multiple of STREAM_CHUNK_UNITS. */
template <bool NT>
__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_stream_gather_kernel(const uint8_t *__restrict__ src, const uint4 *__restrict__ piece, const uint64_t *__restrict__ piece_dst, uint64_t n,
                         uint64_t units, uint64_t span, uint8_t *__restrict__ dst)
{
    const uint32_t lane = threadIdx.x & (KMP_WAVE - 1u);
    const uint64_t w = (uint64_t)blockIdx.x * KMP_BLOCK_WAVES + (threadIdx.x >> 6);
    const uint64_t u_end = min(units, (w + 1u) * span);
    uint32_t p_wave = 0u;                                            /* a piece at or before the one of the round's first unit */
    for (uint64_t u0 = w * span; u0 < u_end; u0 += STREAM_CHUNK_UNITS) {
        u32x4 v[STREAM_UNROLL];
        uint32_t p_first = p_wave;
#pragma unroll
        for (uint32_t r = 0; r < STREAM_UNROLL; ++r) {
            const uint64_t u = u0 + (uint64_t)r * KMP_WAVE + lane;
            v[r] = (u32x4)(0u);
            if (u < u_end) {
                const uint64_t d = u * 16u;
                /* piece_dst[0] == 0 <= d.  Pieces that start at d and hold no byte are passed over: the last one at d is the one with bytes */
                uint64_t q = advance_piece(piece_dst, n, p_wave, d);
                if (r == 0u) p_first = (uint32_t)q;
                uint64_t pd = piece_dst[q];
                do {                                                 /* while pieces start inside the unit: they are this stream's */
                    const uint4 P = piece[q];
                    /* the first piece starts at or before d and may end before it (the stream's end); a later one starts behind d */
                    if (P.z != 0u && (pd > d || d - pd < P.z)) {
                        const int32_t start = (int32_t)(uint32_t)(d - pd);            /* below depth <= 2^30, or -15 .. -1 */
                        v[r] |= fetch_piece<NT>(src + (((uint64_t)P.y << 32) | P.x), start, 0, (int32_t)P.z);     /* (a member starts its slot) */
                    }
                    if (++q >= n) break;
                    pd = piece_dst[q];
                } while (pd < d + 16u);
            }
        }
#pragma unroll
        for (uint32_t r = 0; r < STREAM_UNROLL; ++r) {
            const uint64_t u = u0 + (uint64_t)r * KMP_WAVE + lane;
            if (u < u_end) store_unit<NT>(dst + u * 16u, v[r]);
        }
        p_wave = __builtin_amdgcn_readfirstlane(p_first);            /* lane 0 holds the round's first unit */
    }
}

uint32_t per_element_blocks(uint64_t n)
{
    return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((n + KMP_BLOCK_THREADS - 1) / KMP_BLOCK_THREADS, 1), STREAM_INDEX_BLOCKS);
}

}  // namespace

size_t kmp_stream_ws_bytes(uint64_t n)
{
    const uint64_t nblk = (n + KMP_SCAN_TILE - 1) / KMP_SCAN_TILE;
    return (size_t)(stream_scan_bytes(n) + 8u * (n + nblk) + 4u * (3u * n + 1u + nblk) + 256u);
}

hipError_t kmp_launch_stream_phase1(const uint32_t *pkt_len, uint64_t n, const uint8_t *sort_buf, uint8_t *ws, unsigned long long *totals,
                                    hipStream_t st)
{
    if (n == 0) return hipSuccess;
    const StreamSorted s = stream_sorted(sort_buf, n);
    const StreamWs w = stream_ws(ws, n);
    const uint64_t nblk = (n + KMP_SCAN_TILE - 1) / KMP_SCAN_TILE;
    hipLaunchKernelGGL(kmp_stream_scan_kernel, dim3((uint32_t)nblk), dim3(KMP_BLOCK_THREADS), 0, st, s.key, s.val, pkt_len, n, w.sum, w.cnt,
                       w.blk_sum, w.blk_cnt);
    hipLaunchKernelGGL(kmp_stream_totals_kernel, dim3(1), dim3(KMP_BLOCK_THREADS), 0, st, w.blk_sum, w.blk_cnt, (uint32_t)nblk, totals);
    return hipGetLastError();
}

hipError_t kmp_launch_stream_records(const void *src_meta, uint64_t n, uint64_t total, uint64_t n_streams, uint32_t depth,
                                     const uint8_t *sort_buf, uint8_t *ws, void *recs, void *meta, unsigned long long *totals, hipStream_t st)
{
    static_assert(sizeof(kmpgpu_stream) == 48 && sizeof(kmpgpu_stream_pos) == 16, "the records of kmpgpu.h");
    if (n == 0) return hipSuccess;
    const StreamSorted s = stream_sorted(sort_buf, n);
    const StreamWs w = stream_ws(ws, n);
    hipLaunchKernelGGL(kmp_stream_heads_kernel, dim3(per_element_blocks(n)), dim3(KMP_BLOCK_THREADS), 0, st, s.key, w.cnt, w.blk_cnt, n, n_streams,
                       w.head_pos);
    hipLaunchKernelGGL(kmp_stream_records_kernel, dim3(per_element_blocks(n_streams)), dim3(KMP_BLOCK_THREADS), 0, st, s.key, s.val,
                       reinterpret_cast<const uint4 *>(src_meta), w.sum, w.blk_sum, w.head_pos, n, total, n_streams, depth,
                       reinterpret_cast<uint64_t *>(recs), w.slen, reinterpret_cast<uint4 *>(meta));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return kmp_launch_repack_phase1(w.slen, n_streams, w.scan, totals, st);  /* kmp_scan_local_kernel + kmp_scan_totals_kernel */
}

hipError_t kmp_launch_stream_index(const uint64_t *src_off, const uint32_t *src_len, uint64_t n, uint64_t total, uint64_t n_streams,
                                   const uint8_t *sort_buf, uint8_t *ws, uint64_t *pkt_off, uint32_t *pkt_len, void *map, void *pieces,
                                   hipStream_t st)
{
    if (n == 0) return hipSuccess;
    const StreamSorted s = stream_sorted(sort_buf, n);
    const StreamWs w = stream_ws(ws, n);
    const uint64_t *loc_off = reinterpret_cast<const uint64_t *>(w.scan), *blk_bytes = loc_off + n_streams;
    uint4 *piece = reinterpret_cast<uint4 *>(pieces);
    hipLaunchKernelGGL(kmp_stream_index_kernel, dim3(per_element_blocks(n)), dim3(KMP_BLOCK_THREADS), 0, st, s.val, src_off, src_len, w.sum,
                       w.blk_sum, w.cnt, w.blk_cnt, w.head_pos, w.slen, loc_off, blk_bytes, n, total, n_streams, pkt_off, pkt_len,
                       reinterpret_cast<uint4 *>(map), piece, reinterpret_cast<uint64_t *>(piece + n));
    return hipGetLastError();
}

hipError_t kmp_launch_stream_gather(const uint8_t *src_arena, const void *pieces, uint64_t n, uint64_t total_bytes, uint8_t *arena,
                                    bool nontemporal, hipStream_t st)
{
    if (n == 0 || total_bytes == 0) return hipSuccess;
    const uint64_t units = total_bytes / 16u, chunks = (units + STREAM_CHUNK_UNITS - 1) / STREAM_CHUNK_UNITS;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((chunks + KMP_BLOCK_WAVES - 1) / KMP_BLOCK_WAVES, STREAM_GATHER_BLOCKS);
    const uint64_t waves = (uint64_t)blocks * KMP_BLOCK_WAVES;
    const uint64_t span = (chunks + waves - 1) / waves * STREAM_CHUNK_UNITS;
    const uint4 *piece = reinterpret_cast<const uint4 *>(pieces);
    const uint64_t *piece_dst = reinterpret_cast<const uint64_t *>(piece + n);
    if (nontemporal)
        hipLaunchKernelGGL(kmp_stream_gather_kernel<true>, dim3(blocks), dim3(KMP_BLOCK_THREADS), 0, st, src_arena, piece, piece_dst, n, units, span,
                           arena);
    else
        hipLaunchKernelGGL(kmp_stream_gather_kernel<false>, dim3(blocks), dim3(KMP_BLOCK_THREADS), 0, st, src_arena, piece, piece_dst, n, units, span,
                           arena);
    return hipGetLastError();
}
