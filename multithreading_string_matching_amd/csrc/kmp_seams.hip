/*
 * kmp_seams.hip -- kmpgpu_load_seams: for every payload that has a predecessor in its flow and direction, the predecessor's last `reach`
 * bytes followed by the payload's first `reach` bytes, as a payload of a packed arena (kmpgpu.h).  gfx950.
 *
 *   kmp_seam_keys_kernel      key[k] = flow_of[k] << 1 | dir(k), val[k] = k; dir from the payload's record and its flow's first one
 *   rocprim::radix_sort_pairs the pairs sorted by key, stably: inside a (flow, direction) the payloads stay in capture order.  The project's
 *                             only use of rocPRIM (header-only, ships with ROCm); no atomic decides an order, so the result does not
 *                             depend on the run
 *   kmp_seam_pred_kernel      at sorted position i: k = val[i] has the predecessor val[i - 1] where the two keys are equal.  pred[k], and
 *                             seam_len[k] = min(reach, L_pred) + min(reach, L_k), or 0xFFFFFFFF ("rejected", as kmp_extract_kernel writes
 *                             it) without a predecessor
 *   kmp_scan_local_kernel, kmp_scan_totals_kernel   of kmp_prep.hip, through kmp_launch_repack_phase1: slot offsets and seam numbers in
 *                             ascending order of `next`, totals = {packed bytes, seams}
 *   kmp_seam_index_kernel     the new index, the kmpgpu_seam records, seam_flow, the metadata, and per seam the 32-byte record the gather
 *                             reads: where its tail and its head lie in the source and how long they are
 *   kmp_seam_gather_kernel    the bytes
 *
 * The gather.  The destination is packed and written as kmp_select_copy_kernel writes its own: a wavefront takes a RUN of up to 64
 * consecutive seams, whose new offsets are the prefix sums of their unit counts, keeps the run's table in its 2 KiB of LDS, and deals the
 * run's 16-byte units to the lanes in order -- contiguous stores whatever the seam boundaries.  What differs is the source: a destination
 * unit is made of up to two pieces, neither of them 16-byte aligned relative to it.  The tail starts at off_prev + L_prev - tail_len, any
 * byte address, and the head, which starts on its slot's first byte, lands at byte tail_len of the seam.  A piece is fetched with ALIGNED
 * 16-byte loads of the source units that hold bytes it needs -- one or two --, brought into place with a byte funnel shift
 * (v_alignbyte_b32), and cleared outside the piece's range in registers; tail and head are then ORed.  An aligned unit that holds a byte of
 * a payload lies inside that payload's slot, so no byte outside the slots of prev and next is read: an unaligned 16-byte load at the
 * tail's start could run past prev's slot, and behind the last slot of a borrowed arena there may be nothing.  Everything behind the
 * seam's end comes out 0x00 because no piece covers it.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>

#include <rocprim/device/device_radix_sort.hpp>

#include "kmpgpu.h"
#include "kmp_device.h"
#include "kmp_launch.h"
#include "kmp_piece_dev.h"

namespace {

typedef kmp_piece::u32x4 seam_u32x4;

constexpr uint32_t SEAM_NONE = 0xFFFFFFFFu;
constexpr uint32_t SEAM_UNROLL = 2;              /* destination units a lane has in flight (up to four loads each) */
constexpr uint32_t SEAM_INDEX_BLOCKS = 1024;     /* grid cap of the per-payload kernels: rounds past 262 144 payloads */
constexpr uint32_t SEAM_GATHER_BLOCKS = 1024;    /* grid cap of the gather (16 wavefronts per CU): rounds past 4 096 runs */
constexpr uint32_t SEAM_RUN_BYTES = 16384;       /* bytes a run should come to */

/* The scan workspace of kmp_prep.hip (kmp_extract_ws_bytes): loc_off[n], blk_bytes[nblk], then the 32-bit arrays poff[n], plen[n],
 * loc_idx[n], blk_cnt[nblk].  The seam lengths take plen's place, as the masked lengths of kmp_select.hip do, and pred[] takes poff's,
 * which the scan does not use. */
struct SeamWs {
    uint64_t *loc_off, *blk_bytes;
    uint32_t *pred, *seam_len, *loc_idx, *blk_cnt;
};
SeamWs seam_ws(uint8_t *ws, uint64_t n)
{
    const uint64_t nblk = (n + KMP_SCAN_TILE - 1) / KMP_SCAN_TILE;
    SeamWs w;
    w.loc_off = reinterpret_cast<uint64_t *>(ws);
    w.blk_bytes = w.loc_off + n;
    w.pred = reinterpret_cast<uint32_t *>(w.blk_bytes + nblk);
    w.seam_len = w.pred + n;
    w.loc_idx = w.seam_len + n;
    w.blk_cnt = w.loc_idx + n;
    return w;
}

/* The sort's buffers in the one allocation the context keeps for them: keys in / out, values in / out, rocPRIM's temporary storage. */
struct SeamSort {
    uint64_t *key_in, *key_out;
    uint32_t *val_in, *val_out;
    void     *tmp;
};
SeamSort seam_sort(uint8_t *buf, uint64_t n)
{
    SeamSort s;
    s.key_in = reinterpret_cast<uint64_t *>(buf);
    s.key_out = s.key_in + n;
    s.val_in = reinterpret_cast<uint32_t *>(s.key_out + n);
    s.val_out = s.val_in + n;
    s.tmp = buf + ((24u * n + 255u) & ~255ull);
    return s;
}

/* the key's bits that can differ: the direction bit and the bits of the largest flow id */
uint32_t seam_key_bits(uint64_t n_flows)
{
    uint32_t b = 1u;
    while (b < 33u && ((n_flows - 1u) >> (b - 1u)) != 0u) ++b;
    return b;
}

hipError_t seam_sort_run(void *tmp, size_t &tmp_bytes, const SeamSort &s, uint64_t n, uint64_t n_flows, hipStream_t st)
{
    return rocprim::radix_sort_pairs(tmp, tmp_bytes, s.key_in, s.key_out, s.val_in, s.val_out, (size_t)n, 0u, seam_key_bits(n_flows), st);
}

/* dir(k): 0 where payload k runs the way its flow's first payload does.  The record's first three words are src_ip, dst_ip and the two
 * ports: they are the two endpoints.  A directed flow's payloads all agree with the first one, and so do those of a flow whose two
 * endpoints are equal. */
__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_seam_keys_kernel(const uint4 *__restrict__ meta, const uint32_t *__restrict__ flow_of, const uint4 *__restrict__ flow_recs, uint64_t n,
                     uint64_t *__restrict__ key, uint32_t *__restrict__ val)
{
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (uint64_t)gridDim.x * blockDim.x) {
        const uint4 M = meta[k];
        const uint32_t f = flow_of[k];
        const uint4 F = flow_recs[(uint64_t)f * 3u + 2u];           /* kmpgpu_flow.first: the third 16 bytes of the 48 */
        const uint32_t dir = (((M.x ^ F.x) | (M.y ^ F.y) | (M.z ^ F.z)) != 0u) ? 1u : 0u;       /* (no short circuit: one load per record) */
        key[k] = (uint64_t)f << 1 | dir;
        val[k] = (uint32_t)k;
    }
}

__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_seam_pred_kernel(const uint64_t *__restrict__ key, const uint32_t *__restrict__ val, const uint32_t *__restrict__ pkt_len, uint64_t n,
                     uint32_t reach, uint32_t *__restrict__ pred, uint32_t *__restrict__ seam_len)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t k = val[i];
        uint32_t p = SEAM_NONE, l = 0xFFFFFFFFu;
        if (i > 0 && key[i - 1] == key[i]) {
            p = val[i - 1];
            l = min(reach, pkt_len[p]) + min(reach, pkt_len[k]);
        }
        pred[k] = p;
        seam_len[k] = l;
    }
}

/* Payload k of the source with a predecessor is `next` of seam j. */
__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_seam_index_kernel(const uint64_t *__restrict__ src_off, const uint32_t *__restrict__ src_len, const uint4 *__restrict__ src_meta,
                      const uint32_t *__restrict__ flow_of, const uint32_t *__restrict__ pred, const uint32_t *__restrict__ seam_len,
                      const uint64_t *__restrict__ loc_off, const uint32_t *__restrict__ loc_idx, const uint64_t *__restrict__ blk_bytes,
                      const uint32_t *__restrict__ blk_cnt, uint64_t n, uint32_t reach, uint64_t *__restrict__ pkt_off,
                      uint32_t *__restrict__ pkt_len, uint64_t *__restrict__ seams, uint32_t *__restrict__ seam_flow, uint4 *__restrict__ meta,
                      uint4 *__restrict__ recs)
{
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t l = seam_len[k];
        if (l == 0xFFFFFFFFu) continue;
        const uint64_t blk = k / KMP_SCAN_TILE;
        const uint64_t j = (uint64_t)blk_cnt[blk] + loc_idx[k];
        const uint32_t p = pred[k];
        const uint32_t Lp = src_len[p], tail = min(reach, Lp), head = l - tail;
        const uint64_t ts = src_off[p] + Lp - tail, hs = src_off[k];
        pkt_off[j] = blk_bytes[blk] + loc_off[k];
        pkt_len[j] = l;
        seams[3u * j] = p;                                           /* kmpgpu_seam: prev, next, tail_len | head_len << 32 */
        seams[3u * j + 1u] = k;
        seams[3u * j + 2u] = (uint64_t)head << 32 | tail;
        seam_flow[j] = flow_of[k];
        meta[j] = src_meta[k];
        recs[2u * j] = make_uint4((uint32_t)ts, (uint32_t)(ts >> 32), tail, head);
        recs[2u * j + 1u] = make_uint4((uint32_t)hs, (uint32_t)(hs >> 32), 0u, 0u);
    }
}

/* load_unit / store_unit / fetch_piece: kmp_piece_dev.h, which the gathers of the derived arenas share */
using kmp_piece::fetch_piece;
using kmp_piece::load_unit;
using kmp_piece::store_unit;

template <bool NT>
__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_seam_gather_kernel(const uint8_t *__restrict__ src, const uint64_t *__restrict__ new_off, const uint4 *__restrict__ recs, uint64_t n,
                       uint64_t total, uint32_t run, uint8_t *__restrict__ dst)
{
    __shared__ uint64_t s_off[KMP_BLOCK_WAVES][KMP_WAVE];          /* new offset of seam i of the run; ~0 behind the run's end */
    __shared__ uint64_t s_tail[KMP_BLOCK_WAVES][KMP_WAVE], s_head[KMP_BLOCK_WAVES][KMP_WAVE];      /* where the two pieces start in src */
    __shared__ uint32_t s_tl[KMP_BLOCK_WAVES][KMP_WAVE], s_hl[KMP_BLOCK_WAVES][KMP_WAVE];          /* tail_len, head_len */
    const uint32_t lane = threadIdx.x & (KMP_WAVE - 1u), wid = threadIdx.x >> 6;
    const uint64_t n_runs = (n + run - 1u) / run;
    for (uint64_t r = (uint64_t)blockIdx.x * KMP_BLOCK_WAVES + wid; r < n_runs; r += (uint64_t)gridDim.x * KMP_BLOCK_WAVES) {
        const uint64_t j0 = r * run, j = j0 + lane;
        uint64_t off = ~0ull, ts = 0ull, hs = 0ull;
        uint32_t tl = 0u, hl = 0u;
        if (lane < run && j < n) {
            const uint4 a = recs[2u * j], b = recs[2u * j + 1u];
            off = new_off[j];
            ts = ((uint64_t)a.y << 32) | a.x; tl = a.z; hl = a.w;
            hs = ((uint64_t)b.y << 32) | b.x;
        }
        /* the wavefront's own LDS: its DS instructions execute in order, the barriers keep the compiler from moving them */
        __builtin_amdgcn_wave_barrier();
        s_off[wid][lane] = off; s_tail[wid][lane] = ts; s_head[wid][lane] = hs; s_tl[wid][lane] = tl; s_hl[wid][lane] = hl;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const uint64_t base = new_off[j0];
        const uint64_t end = (j0 + run < n) ? new_off[j0 + run] : total;
        for (uint64_t d0 = base + (uint64_t)lane * 16u; d0 - lane * 16u < end; d0 += (uint64_t)SEAM_UNROLL * KMP_WAVE * 16u) {
            seam_u32x4 v[SEAM_UNROLL];
#pragma unroll
            for (uint32_t u = 0; u < SEAM_UNROLL; ++u) {
                const uint64_t d = d0 + (uint64_t)u * KMP_WAVE * 16u;
                v[u] = (seam_u32x4)(0u);
                if (d < end) {
                    uint32_t p = 0u;                                 /* the last seam of the run that starts at or before d */
#pragma unroll
                    for (uint32_t step = KMP_WAVE / 2u; step; step >>= 1)
                        if (s_off[wid][p + step] <= d) p += step;
                    const uint64_t rel64 = d - s_off[wid][p];
                    const uint32_t T = s_tl[wid][p], H = s_hl[wid][p];
                    if (rel64 < (uint64_t)T + H) {                   /* (an empty seam's slot, or nothing: zeros) */
                        const int32_t rel = (int32_t)rel64;          /* below 2 x 98 */
                        const uint64_t t0 = s_tail[wid][p];
                        const int32_t ta = (int32_t)(t0 & 15u);      /* the tail in the coordinates of the aligned unit it starts in */
                        const seam_u32x4 vt = fetch_piece<NT>(src + (t0 - (uint32_t)ta), ta + rel, ta, ta + (int32_t)T);
                        const seam_u32x4 vh = fetch_piece<NT>(src + s_head[wid][p], rel - (int32_t)T, 0, (int32_t)H);
                        v[u] = vt | vh;
                    }
                }
            }
#pragma unroll
            for (uint32_t u = 0; u < SEAM_UNROLL; ++u) {
                const uint64_t d = d0 + (uint64_t)u * KMP_WAVE * 16u;
                if (d < end) store_unit<NT>(dst + d, v[u]);
            }
        }
        __builtin_amdgcn_wave_barrier();                             /* the next run's table goes over this one */
    }
}

uint32_t per_payload_blocks(uint64_t n)
{
    return (uint32_t)std::min<uint64_t>((n + KMP_BLOCK_THREADS - 1) / KMP_BLOCK_THREADS, SEAM_INDEX_BLOCKS);
}

}  // namespace

size_t kmp_seam_sort_bytes(uint64_t n, uint64_t n_flows)
{
    if (n == 0) return 0;
    size_t tmp = 0;
    const SeamSort s = {nullptr, nullptr, nullptr, nullptr, nullptr};        /* a size query: rocPRIM looks at no pointer */
    if (seam_sort_run(nullptr, tmp, s, n, n_flows, nullptr) != hipSuccess) return 0;
    return (size_t)((24u * n + 255u) & ~255ull) + tmp + 256u;
}

hipError_t kmp_launch_seam_keys(const void *meta, const uint32_t *flow_of, const void *flow_recs, uint64_t n, uint8_t *sort_buf, hipStream_t st)
{
    static_assert(sizeof(kmpgpu_flow) == 48 && sizeof(kmpgpu_pkt_meta) == 16, "kmpgpu_flow.first is the third 16 bytes of a 48-byte record");
    if (n == 0) return hipSuccess;
    const SeamSort s = seam_sort(sort_buf, n);
    hipLaunchKernelGGL(kmp_seam_keys_kernel, dim3(per_payload_blocks(n)), dim3(KMP_BLOCK_THREADS), 0, st, reinterpret_cast<const uint4 *>(meta),
                       flow_of, reinterpret_cast<const uint4 *>(flow_recs), n, s.key_in, s.val_in);
    return hipGetLastError();
}

hipError_t kmp_launch_seam_sort(uint64_t n, uint64_t n_flows, uint8_t *sort_buf, size_t sort_bytes, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    const SeamSort s = seam_sort(sort_buf, n);
    const size_t used = (size_t)(static_cast<uint8_t *>(s.tmp) - sort_buf);
    if (sort_bytes < used) return hipErrorInvalidValue;
    size_t tmp = sort_bytes - used;
    return seam_sort_run(s.tmp, tmp, s, n, n_flows, st);
}

hipError_t kmp_launch_seam_phase1(const uint32_t *pkt_len, uint64_t n, uint32_t reach, const uint8_t *sort_buf, uint8_t *ws,
                                  unsigned long long *totals, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    const SeamSort s = seam_sort(const_cast<uint8_t *>(sort_buf), n);
    const SeamWs w = seam_ws(ws, n);
    hipLaunchKernelGGL(kmp_seam_pred_kernel, dim3(per_payload_blocks(n)), dim3(KMP_BLOCK_THREADS), 0, st, s.key_out, s.val_out, pkt_len, n, reach,
                       w.pred, w.seam_len);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return kmp_launch_repack_phase1(w.seam_len, n, ws, totals, st);          /* kmp_scan_local_kernel + kmp_scan_totals_kernel */
}

hipError_t kmp_launch_seam_index(const uint64_t *src_off, const uint32_t *src_len, const void *src_meta, const uint32_t *flow_of, uint64_t n,
                                 uint32_t reach, uint8_t *ws, uint64_t *pkt_off, uint32_t *pkt_len, void *seams, uint32_t *seam_flow, void *meta,
                                 void *recs, hipStream_t st)
{
    static_assert(sizeof(kmpgpu_seam) == 24, "kmpgpu_seam is three 64-bit words");
    if (n == 0) return hipSuccess;
    const SeamWs w = seam_ws(ws, n);
    hipLaunchKernelGGL(kmp_seam_index_kernel, dim3(per_payload_blocks(n)), dim3(KMP_BLOCK_THREADS), 0, st, src_off, src_len,
                       reinterpret_cast<const uint4 *>(src_meta), flow_of, w.pred, w.seam_len, w.loc_off, w.loc_idx, w.blk_bytes, w.blk_cnt, n,
                       reach, pkt_off, pkt_len, reinterpret_cast<uint64_t *>(seams), seam_flow, reinterpret_cast<uint4 *>(meta),
                       reinterpret_cast<uint4 *>(recs));
    return hipGetLastError();
}

hipError_t kmp_launch_seam_gather(const uint8_t *src_arena, const uint64_t *pkt_off, const void *recs, uint64_t n_seams, uint64_t total_bytes,
                                  uint8_t *arena, bool nontemporal, hipStream_t st)
{
    if (n_seams == 0) return hipSuccess;
    /* seams per run: what brings an average run to SEAM_RUN_BYTES, a power of two up to 64 */
    const uint64_t avg = std::max<uint64_t>(total_bytes / n_seams, 16);
    uint32_t run = KMP_WAVE;
    while (run > 1u && (uint64_t)run * avg > SEAM_RUN_BYTES) run >>= 1;
    const uint64_t n_runs = (n_seams + run - 1) / run;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((n_runs + KMP_BLOCK_WAVES - 1) / KMP_BLOCK_WAVES, SEAM_GATHER_BLOCKS);
    if (nontemporal)
        hipLaunchKernelGGL(kmp_seam_gather_kernel<true>, dim3(blocks), dim3(KMP_BLOCK_THREADS), 0, st, src_arena, pkt_off, (const uint4 *)recs,
                           n_seams, total_bytes, run, arena);
    else
        hipLaunchKernelGGL(kmp_seam_gather_kernel<false>, dim3(blocks), dim3(KMP_BLOCK_THREADS), 0, st, src_arena, pkt_off, (const uint4 *)recs,
                           n_seams, total_bytes, run, arena);
    return hipGetLastError();
}
