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
 *   kmp_scan_local_kernel, kmp_scan_totals_kernel   of kmp_prep.hip, through kmp_launch_compact_scan: slot offsets and seam numbers in
 *                             ascending order of `next`, totals = {packed bytes, seams}
 *   kmp_seam_index_kernel     the new index, the kmpgpu_seam records, seam_flow, the metadata, and per seam the 32-byte record the gather
 *                             reads: where its tail and its head lie in the source and how long they are
 *   kmp_seam_gather_kernel    the bytes
 *
 * The gather.  Its shape -- a wavefront per RUN of up to 64 consecutive seams, the run's 16-byte units dealt to the lanes in order -- is the
 * compacting skeleton's (gather_runs: kmp_compact_dev.h).  What is this file's own is the source: a destination
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
#include "kmp_compact_dev.h"

namespace {

using namespace kmp_unit;     /* kmp_compact_dev.h: gather_runs; kmp_unit_dev.h: the unit */
using kmp_piece::fetch_piece;

constexpr uint32_t SEAM_NONE = 0xFFFFFFFFu;

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

struct SeamRec { uint4 a, b; };          /* the 32-byte record of a seam: {tail address, tail_len, head_len}, {head address} */

template <bool NT>
__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_seam_gather_kernel(const uint8_t *__restrict__ src, const uint64_t *__restrict__ new_off, const uint4 *__restrict__ recs, uint64_t n,
                       uint64_t total, uint32_t run, uint8_t *__restrict__ dst)
{
    __shared__ uint64_t s_tail[KMP_BLOCK_WAVES][KMP_WAVE], s_head[KMP_BLOCK_WAVES][KMP_WAVE];      /* where the two pieces start in src */
    __shared__ uint32_t s_tl[KMP_BLOCK_WAVES][KMP_WAVE], s_hl[KMP_BLOCK_WAVES][KMP_WAVE];          /* tail_len, head_len */
    const uint32_t lane = threadIdx.x & (KMP_WAVE - 1u), wid = threadIdx.x >> 6;
    gather_runs<NT, 2>(new_off, n, total, run, dst,
        [&](uint64_t j, bool in) {
            SeamRec r = {make_uint4(0u, 0u, 0u, 0u), make_uint4(0u, 0u, 0u, 0u)};
            if (in) { r.a = recs[2u * j]; r.b = recs[2u * j + 1u]; }
            return r;
        },
        [&](const SeamRec &r) {
            const uint4 a = r.a, b = r.b;
            s_tail[wid][lane] = ((uint64_t)a.y << 32) | a.x; s_tl[wid][lane] = a.z; s_hl[wid][lane] = a.w;
            s_head[wid][lane] = ((uint64_t)b.y << 32) | b.x;
        },
        [&](uint32_t p, uint64_t rel64, uint32_t &) {
            const uint32_t T = s_tl[wid][p], H = s_hl[wid][p];
            if (rel64 >= (uint64_t)T + H) return (u32x4)(0u);        /* (an empty seam's slot, or nothing: zeros) */
            const int32_t rel = (int32_t)rel64;                      /* below 2 x 98 */
            const uint64_t t0 = s_tail[wid][p];
            const int32_t ta = (int32_t)(t0 & 15u);                  /* the tail in the coordinates of the aligned unit it starts in */
            const u32x4 vt = fetch_piece<NT>(src + (t0 - (uint32_t)ta), ta + rel, ta, ta + (int32_t)T);
            const u32x4 vh = fetch_piece<NT>(src + s_head[wid][p], rel - (int32_t)T, 0, (int32_t)H);
            return vt | vh;
        });
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
    hipLaunchKernelGGL(kmp_seam_keys_kernel, dim3(kmp_item_blocks(n)), dim3(KMP_BLOCK_THREADS), 0, st, reinterpret_cast<const uint4 *>(meta),
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
    const kmp_compact_view w = kmp_compact_ws(ws, n);       /* aux: pred[] */
    hipLaunchKernelGGL(kmp_seam_pred_kernel, dim3(kmp_item_blocks(n)), dim3(KMP_BLOCK_THREADS), 0, st, s.key_out, s.val_out, pkt_len, n, reach,
                       w.aux, w.len);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return kmp_launch_compact_scan(n, ws, totals, st);
}

hipError_t kmp_launch_seam_index(const uint64_t *src_off, const uint32_t *src_len, const void *src_meta, const uint32_t *flow_of, uint64_t n,
                                 uint32_t reach, uint8_t *ws, uint64_t *pkt_off, uint32_t *pkt_len, void *seams, uint32_t *seam_flow, void *meta,
                                 void *recs, hipStream_t st)
{
    static_assert(sizeof(kmpgpu_seam) == 24, "kmpgpu_seam is three 64-bit words");
    if (n == 0) return hipSuccess;
    const kmp_compact_view w = kmp_compact_ws(ws, n);       /* aux: pred[] */
    hipLaunchKernelGGL(kmp_seam_index_kernel, dim3(kmp_item_blocks(n)), dim3(KMP_BLOCK_THREADS), 0, st, src_off, src_len,
                       reinterpret_cast<const uint4 *>(src_meta), flow_of, w.aux, w.len, w.loc_off, w.loc_idx, w.blk_bytes, w.blk_cnt, n,
                       reach, pkt_off, pkt_len, reinterpret_cast<uint64_t *>(seams), seam_flow, reinterpret_cast<uint4 *>(meta),
                       reinterpret_cast<uint4 *>(recs));
    return hipGetLastError();
}

hipError_t kmp_launch_seam_gather(const uint8_t *src_arena, const uint64_t *pkt_off, const void *recs, uint64_t n_seams, uint64_t total_bytes,
                                  uint8_t *arena, bool nontemporal, hipStream_t st)
{
    if (n_seams == 0) return hipSuccess;
    const kmp_run_shape rs = kmp_run_shape_of(n_seams, total_bytes);
    hipLaunchKernelGGL(nontemporal ? kmp_seam_gather_kernel<true> : kmp_seam_gather_kernel<false>, dim3(rs.blocks), dim3(KMP_BLOCK_THREADS), 0, st,
                       src_arena, pkt_off, (const uint4 *)recs, n_seams, total_bytes, rs.run, arena);
    return hipGetLastError();
}
