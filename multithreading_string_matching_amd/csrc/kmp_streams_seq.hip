/*
 * kmp_streams_seq.hip -- kmpgpu_load_streams_ordered: the streams of kmpgpu_load_streams with the members of every TCP stream in SEQUENCE
 * order, bytes already delivered dropped and holes closed (kmpgpu.h).  gfx950.
 *
 * The segments of the sorted order do not depend on the order inside a segment, so the front runs as it is: kmp_seam_keys_kernel,
 * rocprim::radix_sort_pairs and kmp_stream_scan_kernel / kmp_stream_totals_kernel of kmp_seams.hip and kmp_streams.hip leave
 * (flow << 1 | dir, k) sorted, the tile-local head counts and the sums of the members' lengths.  Then, here:
 *
 *   kmp_sseq_heads_kernel       head_pos[s] = the sorted position stream s starts at (kmp_stream_heads_kernel; that file's code object stays)
 *   kmp_sseq_keys_kernel        at sorted position i: key2 = key << 32 | (tcp ? rel + 2^31 : 0), rel measured against the stream's first
 *                               captured member val[head_pos[s]]; per stream tcp[s]
 *   rocprim::radix_sort_pairs   (key2, val) sorted over the bits in use, stably: every segment in (off, k) order, its head holds min rel
 *   kmp_sseq_max_scan_kernel    the tile-local exclusive running MAXIMUM of stream << 33 | end (end = off + L < 2^33; 0 for a stream that is
 *   kmp_sseq_max_totals_kernel  not TCP): streams ascend, so the plain maximum is the segmented one
 *   kmp_sseq_take_scan_kernel   with the maximum complete: skip, and the tile-local exclusive sum of take (64 bits) and count of gaps
 *   kmp_sseq_take_totals_kernel the tiles' totals scanned in place
 *   kmp_sseq_records_kernel     per stream: kmpgpu_stream, kmpgpu_stream_order, len = min(sum take, depth), meta[s] = src.meta[first_packet]
 *   kmp_scan_local_kernel, kmp_scan_totals_kernel   of kmp_prep.hip, through kmp_launch_repack_phase1 over len[]: the slot offsets
 *   kmp_sseq_index_kernel       pkt_off, pkt_len; per ordered position: map, seg, and the PIECE {source address, take in front of the cut, skip}
 *   kmp_sseq_gather_kernel      the bytes: kmp_stream_gather_kernel with a fetch that starts `skip` bytes inside the member
 *
 * The sum of take needs every skip, and a skip needs the maximum across tiles, so the sums are a second small pass, not a second quantity of
 * the first.  The tallies of a stream are differences at head_pos[]: sum take and gaps from the second pass, sum L from kmp_stream_scan_kernel
 * (dup_bytes = sum L - sum take), and gap_bytes = the stream's last maximum - sum take, because every sequence offset below the maximum is
 * either kept once or lies in a gap.  No atomic decides a value anywhere.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include <rocprim/device/device_radix_sort.hpp>

#include "kmpgpu.h"
#include "kmp_device.h"
#include "kmp_launch.h"
#include "kmp_piece_dev.h"

namespace {

using kmp_piece::u32x4;

constexpr uint32_t SSEQ_UNROLL = 1;               /* as kmp_streams.hip: one unit per lane in flight, parallelism from wavefronts */
constexpr uint32_t SSEQ_INDEX_BLOCKS = 1024;      /* grid cap of the per-payload and per-stream kernels: rounds past 262 144 elements */
constexpr uint32_t SSEQ_GATHER_BLOCKS = 2048;
constexpr uint64_t SSEQ_CHUNK_UNITS = (uint64_t)SSEQ_UNROLL * KMP_WAVE;
constexpr uint64_t SSEQ_END_MASK = (1ull << 33) - 1u;

/* What the front left, as kmp_streams.hip lays it out (stream_sorted, stream_ws there): the sorted pairs inside the sort buffer, and in the
 * workspace the scan area of kmp_launch_repack_phase1, then sum[n], blk_sum[nblk], head_pos[n + 1], slen[n], cnt[n], blk_cnt[nblk]. */
struct Front {
    const uint64_t *key; const uint32_t *val;
    uint8_t  *scan;
    uint64_t *sum, *blk_sum;
    uint32_t *head_pos, *slen, *cnt, *blk_cnt;
};
Front front(const uint8_t *sort_buf, uint8_t *ws, uint64_t n)
{
    const uint64_t nblk = (n + KMP_SCAN_TILE - 1) / KMP_SCAN_TILE;
    Front f;
    f.key = reinterpret_cast<const uint64_t *>(sort_buf) + n;
    f.val = reinterpret_cast<const uint32_t *>(f.key + n) + n;
    f.scan = ws;
    f.sum = reinterpret_cast<uint64_t *>(ws + (((uint64_t)kmp_extract_ws_bytes(n) + 255u) & ~255ull));
    f.blk_sum = f.sum + n;
    f.head_pos = reinterpret_cast<uint32_t *>(f.blk_sum + nblk);
    f.slen = f.head_pos + n + 1u;
    f.cnt = f.slen + n;
    f.blk_cnt = f.cnt + n;
    return f;
}

/* This file's own workspace.  key_in is dead once the sort has run: the running maxima take its place. */
struct SeqWs {
    uint64_t *key_in, *key2, *mx, *blk_mx, *tsum, *blk_tsum, *grand;      /* [n], [n], = key_in, [nblk], [n], [nblk], [4] */
    uint32_t *val2, *skip, *gcnt, *blk_gcnt, *tcp;                          /* [n], [n], [n], [nblk], [n] (per stream) */
    void     *tmp;
};
uint64_t seq_fixed_bytes(uint64_t n)
{
    const uint64_t nblk = (n + KMP_SCAN_TILE - 1) / KMP_SCAN_TILE;
    return (8u * (3u * n + 2u * nblk + 4u) + 4u * (4u * n + nblk) + 255u) & ~255ull;
}
SeqWs seq_ws(uint8_t *ws2, uint64_t n)
{
    const uint64_t nblk = (n + KMP_SCAN_TILE - 1) / KMP_SCAN_TILE;
    SeqWs w;
    w.key_in = reinterpret_cast<uint64_t *>(ws2);
    w.mx = w.key_in;
    w.key2 = w.key_in + n;
    w.tsum = w.key2 + n;
    w.blk_mx = w.tsum + n;
    w.blk_tsum = w.blk_mx + nblk;
    w.grand = w.blk_tsum + nblk;
    w.val2 = reinterpret_cast<uint32_t *>(w.grand + 4u);
    w.skip = w.val2 + n;
    w.gcnt = w.skip + n;
    w.tcp = w.gcnt + n;
    w.blk_gcnt = w.tcp + n;
    w.tmp = ws2 + seq_fixed_bytes(n);
    return w;
}

/* the bits of key2 that can differ: 32 of the sequence offset, the direction bit and the bits of the largest flow id (kmp_seams.hip) */
uint32_t seq_key_bits(uint64_t n_flows)
{
    uint32_t b = 1u;
    while (b < 32u && ((n_flows - 1u) >> (b - 1u)) != 0u) ++b;
    return 32u + b;
}

hipError_t seq_sort_run(void *tmp, size_t &tmp_bytes, const uint64_t *key_in, uint64_t *key_out, const uint32_t *val_in, uint32_t *val_out,
                        uint64_t n, uint64_t n_flows, hipStream_t st)
{
    return rocprim::radix_sort_pairs(tmp, tmp_bytes, key_in, key_out, val_in, val_out, (size_t)n, 0u, seq_key_bits(n_flows), st);
}

/* the stream of sorted position i */
__device__ __forceinline__ uint64_t stream_of(const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ blk_cnt, uint64_t i)
{
    return (uint64_t)blk_cnt[i / KMP_SCAN_TILE] + cnt[i] - 1u;
}

__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_sseq_heads_kernel(const uint64_t *__restrict__ key, const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ blk_cnt, uint64_t n,
                      uint64_t n_streams, uint32_t *__restrict__ head_pos)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        if (i == 0 || key[i - 1] != key[i]) head_pos[stream_of(cnt, blk_cnt, i)] = (uint32_t)i;
        if (i == n - 1u) head_pos[n_streams] = (uint32_t)n;
    }
}

__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_sseq_keys_kernel(const uint64_t *__restrict__ key, const uint32_t *__restrict__ val, const uint4 *__restrict__ src_meta,
                     const uint32_t *__restrict__ seq, const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ blk_cnt,
                     const uint32_t *__restrict__ head_pos, uint64_t n, uint64_t *__restrict__ key2, uint32_t *__restrict__ tcp)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t s = stream_of(cnt, blk_cnt, i);
        const uint32_t h = head_pos[s], k0 = val[h];
        const uint32_t is_tcp = (src_meta[k0].w & 0xFFu) == 6u ? 1u : 0u;                /* kmpgpu_pkt_meta.proto */
        const uint32_t lo = is_tcp ? (seq[val[i]] - seq[k0]) ^ 0x80000000u : 0u;         /* rel + 2^31 */
        key2[i] = key[i] << 32 | lo;
        if (i == h) tcp[s] = is_tcp;
    }
}

/* What the two scans see at ordered position j < n: the stream, its head, the member's length and sequence offset. */
struct Member { uint64_t s; uint32_t h, L, off, tcp; };
__device__ __forceinline__ Member member_at(const uint64_t *__restrict__ key2, const uint32_t *__restrict__ val2,
                                            const uint32_t *__restrict__ pkt_len, const uint32_t *__restrict__ cnt,
                                            const uint32_t *__restrict__ blk_cnt, const uint32_t *__restrict__ head_pos,
                                            const uint32_t *__restrict__ tcp, uint64_t j)
{
    Member m;
    m.s = stream_of(cnt, blk_cnt, j);
    m.h = head_pos[m.s];
    m.tcp = tcp[m.s];
    m.L = pkt_len[val2[j]];
    m.off = m.tcp ? (uint32_t)key2[j] - (uint32_t)key2[m.h] : 0u;
    return m;
}

__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_sseq_max_scan_kernel(const uint64_t *__restrict__ key2, const uint32_t *__restrict__ val2, const uint32_t *__restrict__ pkt_len,
                         const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ blk_cnt, const uint32_t *__restrict__ head_pos,
                         const uint32_t *__restrict__ tcp, uint64_t n, uint64_t *__restrict__ mx, uint64_t *__restrict__ blk_mx)
{
    __shared__ uint64_t s_m[KMP_BLOCK_THREADS];
    const uint64_t base = (uint64_t)blockIdx.x * KMP_SCAN_TILE + (uint64_t)threadIdx.x * KMP_SCAN_ITEMS;
    uint64_t m[KMP_SCAN_ITEMS], tm = 0;
#pragma unroll
    for (uint32_t i = 0; i < KMP_SCAN_ITEMS; i++) {
        const uint64_t j = base + i;
        uint64_t v = 0;
        if (j < n) {
            const Member M = member_at(key2, val2, pkt_len, cnt, blk_cnt, head_pos, tcp, j);
            v = M.s << 33 | (M.tcp ? (uint64_t)M.off + M.L : 0ull);
        }
        m[i] = tm;                                                     /* exclusive */
        tm = max(tm, v);
    }
    s_m[threadIdx.x] = tm;
    __syncthreads();
    for (uint32_t d = 1; d < KMP_BLOCK_THREADS; d <<= 1) {            /* Hillis-Steele inclusive scan of the thread maxima */
        const uint64_t v = threadIdx.x >= d ? s_m[threadIdx.x - d] : 0ull;
        __syncthreads();
        s_m[threadIdx.x] = max(s_m[threadIdx.x], v);
        __syncthreads();
    }
    const uint64_t em = threadIdx.x ? s_m[threadIdx.x - 1u] : 0ull;
#pragma unroll
    for (uint32_t i = 0; i < KMP_SCAN_ITEMS; i++)
        if (base + i < n) mx[base + i] = max(em, m[i]);
    if (threadIdx.x == KMP_BLOCK_THREADS - 1u) blk_mx[blockIdx.x] = s_m[threadIdx.x];
}

/* One block: exclusive maximum scan of the tile maxima in place; grand[0] = the maximum of all. */
__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_sseq_max_totals_kernel(uint64_t *__restrict__ blk_mx, uint32_t nblk, uint64_t *__restrict__ grand)
{
    __shared__ uint64_t s_m[KMP_BLOCK_THREADS];
    uint64_t cm = 0;
    for (uint32_t base = 0; base < nblk; base += KMP_BLOCK_THREADS) {
        const uint32_t i = base + threadIdx.x;
        s_m[threadIdx.x] = i < nblk ? blk_mx[i] : 0ull;
        __syncthreads();
        for (uint32_t d = 1; d < KMP_BLOCK_THREADS; d <<= 1) {
            const uint64_t v = threadIdx.x >= d ? s_m[threadIdx.x - d] : 0ull;
            __syncthreads();
            s_m[threadIdx.x] = max(s_m[threadIdx.x], v);
            __syncthreads();
        }
        if (i < nblk) blk_mx[i] = max(cm, threadIdx.x ? s_m[threadIdx.x - 1u] : 0ull);
        cm = max(cm, s_m[KMP_BLOCK_THREADS - 1u]);
        __syncthreads();
    }
    if (threadIdx.x == 0u) grand[0] = cm;
}

/* M(k): the exclusive maximum at ordered position j where it belongs to j's stream, otherwise 0 */
__device__ __forceinline__ uint64_t covered_to(const uint64_t *__restrict__ mx, const uint64_t *__restrict__ blk_mx, uint64_t j, uint64_t s)
{
    const uint64_t raw = max(blk_mx[j / KMP_SCAN_TILE], mx[j]);
    return (raw >> 33) == s ? raw & SSEQ_END_MASK : 0ull;
}

__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_sseq_take_scan_kernel(const uint64_t *__restrict__ key2, const uint32_t *__restrict__ val2, const uint32_t *__restrict__ pkt_len,
                          const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ blk_cnt, const uint32_t *__restrict__ head_pos,
                          const uint32_t *__restrict__ tcp, const uint64_t *__restrict__ mx, const uint64_t *__restrict__ blk_mx, uint64_t n,
                          uint32_t *__restrict__ skip, uint64_t *__restrict__ tsum, uint32_t *__restrict__ gcnt,
                          uint64_t *__restrict__ blk_tsum, uint32_t *__restrict__ blk_gcnt)
{
    __shared__ uint64_t s_b[KMP_BLOCK_THREADS];
    __shared__ uint32_t s_c[KMP_BLOCK_THREADS];
    const uint64_t base = (uint64_t)blockIdx.x * KMP_SCAN_TILE + (uint64_t)threadIdx.x * KMP_SCAN_ITEMS;
    uint64_t b[KMP_SCAN_ITEMS], tb = 0;
    uint32_t c[KMP_SCAN_ITEMS], sk[KMP_SCAN_ITEMS], tc = 0;
#pragma unroll
    for (uint32_t i = 0; i < KMP_SCAN_ITEMS; i++) {
        const uint64_t j = base + i;
        uint32_t take = 0u, gap = 0u;
        sk[i] = 0u;
        if (j < n) {
            const Member M = member_at(key2, val2, pkt_len, cnt, blk_cnt, head_pos, tcp, j);
            const uint64_t to = covered_to(mx, blk_mx, j, M.s);
            if (M.tcp) {
                /* ONE signed difference (both below 2^34) for the two tests: covered bytes where positive, a gap where negative.  Written
                 * as `to > off ? min(L, to - off) : 0` beside `off > to`, hipcc -O3 hoists the subtraction with its no-wrap flag out of
                 * the selection and then folds the second comparison to false: no gap was ever counted. */
                const int64_t ahead = (int64_t)to - (int64_t)M.off;
                sk[i] = ahead > 0 ? (ahead < (int64_t)M.L ? (uint32_t)ahead : M.L) : 0u;
                gap = (j != M.h && ahead < 0) ? 1u : 0u;
            }
            take = M.L - sk[i];
        }
        b[i] = tb; c[i] = tc;                                         /* both exclusive */
        tb += take; tc += gap;
    }
    s_b[threadIdx.x] = tb; s_c[threadIdx.x] = tc;
    __syncthreads();
    for (uint32_t d = 1; d < KMP_BLOCK_THREADS; d <<= 1) {
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
        if (base + i < n) { skip[base + i] = sk[i]; tsum[base + i] = eb + b[i]; gcnt[base + i] = ec + c[i]; }
    if (threadIdx.x == KMP_BLOCK_THREADS - 1u) { blk_tsum[blockIdx.x] = s_b[threadIdx.x]; blk_gcnt[blockIdx.x] = s_c[threadIdx.x]; }
}

/* One block: exclusive scan of the tile totals in place; grand[1] = the sum of take, grand[2] = gaps. */
__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_sseq_take_totals_kernel(uint64_t *__restrict__ blk_tsum, uint32_t *__restrict__ blk_gcnt, uint32_t nblk, uint64_t *__restrict__ grand)
{
    __shared__ uint64_t s_b[KMP_BLOCK_THREADS];
    __shared__ uint32_t s_c[KMP_BLOCK_THREADS];
    uint64_t cb = 0, cc = 0;
    for (uint32_t base = 0; base < nblk; base += KMP_BLOCK_THREADS) {
        const uint32_t i = base + threadIdx.x;
        const uint64_t vb0 = i < nblk ? blk_tsum[i] : 0ull;
        const uint32_t vc0 = i < nblk ? blk_gcnt[i] : 0u;
        s_b[threadIdx.x] = vb0; s_c[threadIdx.x] = vc0;
        __syncthreads();
        for (uint32_t d = 1; d < KMP_BLOCK_THREADS; d <<= 1) {
            const uint64_t vb = threadIdx.x >= d ? s_b[threadIdx.x - d] : 0ull;
            const uint32_t vc = threadIdx.x >= d ? s_c[threadIdx.x - d] : 0u;
            __syncthreads();
            s_b[threadIdx.x] += vb; s_c[threadIdx.x] += vc;
            __syncthreads();
        }
        if (i < nblk) { blk_tsum[i] = cb + s_b[threadIdx.x] - vb0; blk_gcnt[i] = (uint32_t)(cc + s_c[threadIdx.x] - vc0); }
        cb += s_b[KMP_BLOCK_THREADS - 1u]; cc += s_c[KMP_BLOCK_THREADS - 1u];
        __syncthreads();
    }
    if (threadIdx.x == 0u) { grand[1] = cb; grand[2] = cc; }
}

/* a tile-local exclusive sum plus its tile's offset at position i <= n */
__device__ __forceinline__ uint64_t sum_at(const uint64_t *__restrict__ sum, const uint64_t *__restrict__ blk_sum, uint64_t i, uint64_t n,
                                           uint64_t total)
{
    return i < n ? blk_sum[i / KMP_SCAN_TILE] + sum[i] : total;
}

__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_sseq_records_kernel(const uint64_t *__restrict__ key, const uint32_t *__restrict__ val, const uint64_t *__restrict__ key2,
                        const uint4 *__restrict__ src_meta, const uint32_t *__restrict__ seq, const uint64_t *__restrict__ sum,
                        const uint64_t *__restrict__ blk_sum, const uint32_t *__restrict__ head_pos, const uint32_t *__restrict__ tcp,
                        const uint64_t *__restrict__ mx, const uint64_t *__restrict__ blk_mx, const uint64_t *__restrict__ tsum,
                        const uint64_t *__restrict__ blk_tsum, const uint32_t *__restrict__ gcnt, const uint32_t *__restrict__ blk_gcnt,
                        const uint64_t *__restrict__ grand, uint64_t n, uint64_t total, uint64_t n_streams, uint32_t depth,
                        uint64_t *__restrict__ recs, uint64_t *__restrict__ orders, uint32_t *__restrict__ slen, uint4 *__restrict__ meta)
{
    for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n_streams; s += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t h = head_pos[s], e = head_pos[s + 1u];
        const uint64_t members = sum_at(sum, blk_sum, e, n, total) - sum_at(sum, blk_sum, h, n, total);
        const uint64_t bytes = sum_at(tsum, blk_tsum, e, n, grand[1]) - sum_at(tsum, blk_tsum, h, n, grand[1]);
        const uint64_t gaps = (e < n ? (uint64_t)blk_gcnt[e / KMP_SCAN_TILE] + gcnt[e] : grand[2]) - ((uint64_t)blk_gcnt[h / KMP_SCAN_TILE] + gcnt[h]);
        const uint64_t last = (e < n ? max(blk_mx[e / KMP_SCAN_TILE], mx[e]) : grand[0]) & SSEQ_END_MASK;      /* of stream s: e - 1 is its member */
        const uint32_t len = (uint32_t)min(bytes, (uint64_t)depth);
        const uint64_t k = key[h];
        const uint32_t first = val[h], is_tcp = tcp[s];
        const uint32_t seq_base = is_tcp ? seq[first] + (((uint32_t)key2[h]) ^ 0x80000000u) : 0u;             /* the sequence number of offset 0 */
        recs[6u * s] = first;                                        /* kmpgpu_stream, as kmp_stream_records_kernel writes it */
        recs[6u * s + 1u] = val[e - 1u];
        recs[6u * s + 2u] = e - h;
        recs[6u * s + 3u] = bytes;
        recs[6u * s + 4u] = (k & 1u) << 32 | (k >> 1);
        recs[6u * s + 5u] = len;
        orders[4u * s] = gaps << 32 | seq_base;                      /* kmpgpu_stream_order: seq_base, n_gaps, gap_bytes, dup_bytes, tcp | 0 << 32 */
        orders[4u * s + 1u] = is_tcp ? last - bytes : 0ull;
        orders[4u * s + 2u] = members - bytes;
        orders[4u * s + 3u] = is_tcp;
        slen[s] = len;
        meta[s] = src_meta[first];
    }
}

__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_sseq_index_kernel(const uint64_t *__restrict__ key2, const uint32_t *__restrict__ val2, const uint64_t *__restrict__ src_off,
                      const uint32_t *__restrict__ src_len, const uint32_t *__restrict__ skip, const uint64_t *__restrict__ tsum,
                      const uint64_t *__restrict__ blk_tsum, const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ blk_cnt,
                      const uint32_t *__restrict__ head_pos, const uint32_t *__restrict__ tcp, const uint32_t *__restrict__ slen,
                      const uint64_t *__restrict__ loc_off, const uint64_t *__restrict__ blk_bytes, uint64_t n, uint64_t n_streams,
                      uint64_t *__restrict__ pkt_off, uint32_t *__restrict__ pkt_len, uint4 *__restrict__ map, uint4 *__restrict__ segs,
                      uint4 *__restrict__ piece, uint64_t *__restrict__ piece_dst)
{
    const uint64_t t0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t s = t0; s < n_streams; s += step) {
        pkt_off[s] = blk_bytes[s / KMP_SCAN_TILE] + loc_off[s];
        pkt_len[s] = slen[s];
    }
    for (uint64_t i = t0; i < n; i += step) {
        const uint32_t k = val2[i];
        const uint64_t s = stream_of(cnt, blk_cnt, i);
        const uint32_t h = head_pos[s];
        const uint64_t pos = (blk_tsum[i / KMP_SCAN_TILE] + tsum[i]) - (blk_tsum[h / KMP_SCAN_TILE] + tsum[h]);
        const uint32_t len = slen[s], L = src_len[k], sk = skip[i];
        const uint32_t off = tcp[s] ? (uint32_t)key2[i] - (uint32_t)key2[h] : 0u;
        /* a member at or behind the cut, or fully covered: no byte, at its place (destinations stay ascending) */
        const uint32_t at = (uint32_t)min(pos, (uint64_t)len), take = min(L - sk, len - at);
        const uint64_t so = src_off[k];
        map[k] = make_uint4((uint32_t)s, 0u, (uint32_t)pos, (uint32_t)(pos >> 32));      /* kmpgpu_stream_pos: stream, 0, pos */
        segs[k] = make_uint4(sk, L - sk, off, 0u);                                        /* kmpgpu_stream_seg: skip, take, seq_off, 0 */
        piece[i] = make_uint4((uint32_t)so, (uint32_t)(so >> 32), take, sk);
        piece_dst[i] = blk_bytes[s / KMP_SCAN_TILE] + loc_off[s] + at;
    }
}

/* load_unit / store_unit / fetch_piece: kmp_piece_dev.h, which the gathers of the derived arenas share */
using kmp_piece::fetch_piece;
using kmp_piece::load_unit;
using kmp_piece::store_unit;

/* The last piece q >= p with piece_dst[q] <= d, given piece_dst[p] <= d: galloping, then halving.  0-byte pieces at or before d -- members
 * behind the cut, and here fully covered retransmissions in the middle of a stream -- are passed over by the search, not walked. */
__device__ __forceinline__ uint32_t advance_piece(const uint64_t *__restrict__ piece_dst, uint64_t n, uint32_t p, uint64_t d)
{
    uint64_t q = p, step = 1;
    while (q + step < n && piece_dst[q + step] <= d) { q += step; step <<= 1; }
    for (step >>= 1; step; step >>= 1)
        if (q + step < n && piece_dst[q + step] <= d) q += step;
    return (uint32_t)q;
}

/* Wavefront w of all W writes the units [w * span, (w + 1) * span) of the arena's `units`, span a multiple of SSEQ_CHUNK_UNITS. */
template <bool NT>
__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_sseq_gather_kernel(const uint8_t *__restrict__ src, const uint4 *__restrict__ piece, const uint64_t *__restrict__ piece_dst, uint64_t n,
                       uint64_t units, uint64_t span, uint8_t *__restrict__ dst)
{
    const uint32_t lane = threadIdx.x & (KMP_WAVE - 1u);
    const uint64_t w = (uint64_t)blockIdx.x * KMP_BLOCK_WAVES + (threadIdx.x >> 6);
    const uint64_t u_end = min(units, (w + 1u) * span);
    uint32_t p_wave = 0u;                                            /* a piece at or before the one of the round's first unit */
    for (uint64_t u0 = w * span; u0 < u_end; u0 += SSEQ_CHUNK_UNITS) {
        u32x4 v[SSEQ_UNROLL];
        uint32_t p_first = p_wave;
#pragma unroll
        for (uint32_t r = 0; r < SSEQ_UNROLL; ++r) {
            const uint64_t u = u0 + (uint64_t)r * KMP_WAVE + lane;
            v[r] = (u32x4)(0u);
            if (u < u_end) {
                const uint64_t d = u * 16u;
                /* piece_dst[0] == 0 <= d */
                uint64_t q = advance_piece(piece_dst, n, p_wave, d);
                if (r == 0u) p_first = (uint32_t)q;
                uint64_t pd = piece_dst[q];
                for (;;) {                                           /* while pieces start inside the unit: they are this stream's */
                    const uint4 P = piece[q];
                    /* the first piece starts at or before d and may end before it (the stream's end); a later one starts behind d */
                    if (P.z != 0u && (pd > d || d - pd < P.z)) {
                        /* the kept bytes are [skip, skip + take) of the member: destination byte pd is its byte `skip` */
                        const int32_t start = (int32_t)(uint32_t)(d - pd) + (int32_t)P.w;
                        v[r] |= fetch_piece<NT>(src + (((uint64_t)P.y << 32) | P.x), start, (int32_t)P.w, (int32_t)(P.w + P.z));
                    }
                    if (++q >= n) break;
                    pd = piece_dst[q];
                    if (pd >= d + 16u) break;
                    /* pieces that share a destination hold no byte, all but the last: the search passes over them (one load where
                     * the next piece starts behind pd), so covered retransmissions and members behind an odd cut are not walked */
                    q = advance_piece(piece_dst, n, (uint32_t)q, pd);
                }
            }
        }
#pragma unroll
        for (uint32_t r = 0; r < SSEQ_UNROLL; ++r) {
            const uint64_t u = u0 + (uint64_t)r * KMP_WAVE + lane;
            if (u < u_end) store_unit<NT>(dst + u * 16u, v[r]);
        }
        p_wave = __builtin_amdgcn_readfirstlane(p_first);            /* lane 0 holds the round's first unit */
    }
}

uint32_t per_element_blocks(uint64_t n)
{
    return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((n + KMP_BLOCK_THREADS - 1) / KMP_BLOCK_THREADS, 1), SSEQ_INDEX_BLOCKS);
}

}  // namespace

size_t kmp_stream_seq_ws_bytes(uint64_t n, uint64_t n_flows)
{
    if (n == 0) return 0;
    size_t tmp = 0;
    if (seq_sort_run(nullptr, tmp, nullptr, nullptr, nullptr, nullptr, n, n_flows, nullptr) != hipSuccess) return 0;     /* a size query */
    return (size_t)(seq_fixed_bytes(n) + tmp + 256u);
}

hipError_t kmp_launch_stream_seq_order(const void *src_meta, const uint32_t *seq, uint64_t n, uint64_t n_streams, uint64_t n_flows,
                                       const uint8_t *sort_buf, uint8_t *ws, uint8_t *ws2, size_t ws2_bytes, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    const Front f = front(sort_buf, ws, n);
    const SeqWs w = seq_ws(ws2, n);
    const size_t used = (size_t)(static_cast<uint8_t *>(w.tmp) - ws2);
    if (ws2_bytes < used) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kmp_sseq_heads_kernel, dim3(per_element_blocks(n)), dim3(KMP_BLOCK_THREADS), 0, st, f.key, f.cnt, f.blk_cnt, n, n_streams,
                       f.head_pos);
    hipLaunchKernelGGL(kmp_sseq_keys_kernel, dim3(per_element_blocks(n)), dim3(KMP_BLOCK_THREADS), 0, st, f.key, f.val,
                       reinterpret_cast<const uint4 *>(src_meta), seq, f.cnt, f.blk_cnt, f.head_pos, n, w.key_in, w.tcp);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    size_t tmp = ws2_bytes - used;
    return seq_sort_run(w.tmp, tmp, w.key_in, w.key2, f.val, w.val2, n, n_flows, st);
}

hipError_t kmp_launch_stream_seq_scans(const uint32_t *pkt_len, uint64_t n, const uint8_t *sort_buf, uint8_t *ws, uint8_t *ws2, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    const Front f = front(sort_buf, ws, n);
    const SeqWs w = seq_ws(ws2, n);
    const uint64_t nblk = (n + KMP_SCAN_TILE - 1) / KMP_SCAN_TILE;
    hipLaunchKernelGGL(kmp_sseq_max_scan_kernel, dim3((uint32_t)nblk), dim3(KMP_BLOCK_THREADS), 0, st, w.key2, w.val2, pkt_len, f.cnt, f.blk_cnt,
                       f.head_pos, w.tcp, n, w.mx, w.blk_mx);
    hipLaunchKernelGGL(kmp_sseq_max_totals_kernel, dim3(1), dim3(KMP_BLOCK_THREADS), 0, st, w.blk_mx, (uint32_t)nblk, w.grand);
    hipLaunchKernelGGL(kmp_sseq_take_scan_kernel, dim3((uint32_t)nblk), dim3(KMP_BLOCK_THREADS), 0, st, w.key2, w.val2, pkt_len, f.cnt, f.blk_cnt,
                       f.head_pos, w.tcp, w.mx, w.blk_mx, n, w.skip, w.tsum, w.gcnt, w.blk_tsum, w.blk_gcnt);
    hipLaunchKernelGGL(kmp_sseq_take_totals_kernel, dim3(1), dim3(KMP_BLOCK_THREADS), 0, st, w.blk_tsum, w.blk_gcnt, (uint32_t)nblk, w.grand);
    return hipGetLastError();
}

hipError_t kmp_launch_stream_seq_records(const void *src_meta, const uint32_t *seq, uint64_t n, uint64_t total, uint64_t n_streams,
                                         uint32_t depth, const uint8_t *sort_buf, uint8_t *ws, uint8_t *ws2, void *recs, void *orders,
                                         void *meta, unsigned long long *totals, hipStream_t st)
{
    static_assert(sizeof(kmpgpu_stream) == 48 && sizeof(kmpgpu_stream_order) == 32 && sizeof(kmpgpu_stream_seg) == 16, "the records of kmpgpu.h");
    if (n == 0) return hipSuccess;
    const Front f = front(sort_buf, ws, n);
    const SeqWs w = seq_ws(ws2, n);
    hipLaunchKernelGGL(kmp_sseq_records_kernel, dim3(per_element_blocks(n_streams)), dim3(KMP_BLOCK_THREADS), 0, st, f.key, f.val, w.key2,
                       reinterpret_cast<const uint4 *>(src_meta), seq, f.sum, f.blk_sum, f.head_pos, w.tcp, w.mx, w.blk_mx, w.tsum, w.blk_tsum,
                       w.gcnt, w.blk_gcnt, w.grand, n, total, n_streams, depth, reinterpret_cast<uint64_t *>(recs),
                       reinterpret_cast<uint64_t *>(orders), f.slen, reinterpret_cast<uint4 *>(meta));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return kmp_launch_repack_phase1(f.slen, n_streams, f.scan, totals, st);  /* kmp_scan_local_kernel + kmp_scan_totals_kernel */
}

hipError_t kmp_launch_stream_seq_index(const uint64_t *src_off, const uint32_t *src_len, uint64_t n, uint64_t n_streams, const uint8_t *sort_buf,
                                       uint8_t *ws, uint8_t *ws2, uint64_t *pkt_off, uint32_t *pkt_len, void *map, void *segs, void *pieces,
                                       hipStream_t st)
{
    if (n == 0) return hipSuccess;
    const Front f = front(sort_buf, ws, n);
    const SeqWs w = seq_ws(ws2, n);
    const uint64_t *loc_off = reinterpret_cast<const uint64_t *>(f.scan), *blk_bytes = loc_off + n_streams;
    uint4 *piece = reinterpret_cast<uint4 *>(pieces);
    hipLaunchKernelGGL(kmp_sseq_index_kernel, dim3(per_element_blocks(n)), dim3(KMP_BLOCK_THREADS), 0, st, w.key2, w.val2, src_off, src_len, w.skip,
                       w.tsum, w.blk_tsum, f.cnt, f.blk_cnt, f.head_pos, w.tcp, f.slen, loc_off, blk_bytes, n, n_streams, pkt_off, pkt_len,
                       reinterpret_cast<uint4 *>(map), reinterpret_cast<uint4 *>(segs), piece, reinterpret_cast<uint64_t *>(piece + n));
    return hipGetLastError();
}

hipError_t kmp_launch_stream_seq_gather(const uint8_t *src_arena, const void *pieces, uint64_t n, uint64_t total_bytes, uint8_t *arena,
                                        bool nontemporal, hipStream_t st)
{
    if (n == 0 || total_bytes == 0) return hipSuccess;
    const uint64_t units = total_bytes / 16u, chunks = (units + SSEQ_CHUNK_UNITS - 1) / SSEQ_CHUNK_UNITS;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((chunks + KMP_BLOCK_WAVES - 1) / KMP_BLOCK_WAVES, SSEQ_GATHER_BLOCKS);
    const uint64_t waves = (uint64_t)blocks * KMP_BLOCK_WAVES;
    const uint64_t span = (chunks + waves - 1) / waves * SSEQ_CHUNK_UNITS;
    const uint4 *piece = reinterpret_cast<const uint4 *>(pieces);
    const uint64_t *piece_dst = reinterpret_cast<const uint64_t *>(piece + n);
    if (nontemporal)
        hipLaunchKernelGGL(kmp_sseq_gather_kernel<true>, dim3(blocks), dim3(KMP_BLOCK_THREADS), 0, st, src_arena, piece, piece_dst, n, units, span,
                           arena);
    else
        hipLaunchKernelGGL(kmp_sseq_gather_kernel<false>, dim3(blocks), dim3(KMP_BLOCK_THREADS), 0, st, src_arena, piece, piece_dst, n, units, span,
                           arena);
    return hipGetLastError();
}
