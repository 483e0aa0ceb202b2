/*
 * kmp_headers.hip -- the header predicates of kmpgpu_scan_headers / kmpgpu_scan_rules on gfx950 (kmpgpu_set_headers, kmpgpu.h), and the
 * two small kernels that carry the per-payload metadata they read beside the index (KMPGPU_OPT_KEEP_META, kmpgpu_load_selected).
 *
 * The header kernel runs behind the marking pass and writes one further row of the hit matrix per predicate:
 *   rows[q][j]     = for the payloads k of word j: predicate q holds for (meta[k], pkt_len[k])
 *   hdr_counts[q]  = the set bits of row q
 *   any[j]         = OR over all predicates of word j
 * Nothing of the text is read: 16 bytes of metadata and 4 bytes of length per payload, once per pass however many predicates there are.
 *
 * Shape: a lane owns a payload, a wavefront owns a column word, a block of four wavefronts owns four consecutive words (256 payloads).
 * Every lane loads its payload's record (one 16-byte load, coalesced: a KiB per wavefront) and its length, and keeps them in registers.
 * The predicates come in tiles of KMP_HDR_TILE: the block copies a tile's 48-byte records into LDS, then every wavefront walks the
 * tile -- the record's address is wavefront-uniform, an LDS broadcast read, and its words go on into scalar registers --, decides its
 * lane's payload without a branch and turns the 64 answers into the row word with one ballot.  A lane whose payload lies at n_pkts or
 * behind answers no, so those bits and the padding word of an odd W come out 0 without a mask.
 * Stores: the four ballots of a (predicate, block) go to LDS, and once the tile is done thread t of the block writes 16 bytes of
 * predicate t / 2: the block's 32 bytes of a row leave in two 16-byte stores of neighbouring lanes, a tile in 4 KiB of them.  (One
 * 8-byte store per (wavefront, predicate) from lane 0 would write the same bytes in four partial sectors at four different times.)
 * The same two threads add up the popcount of their words and one of them adds it to hdr_counts[q]: one atomic per (block, row).  The
 * column OR is kept per wavefront in a scalar over all tiles and ORed into any[j] once at the end, as kmp_rules.hip leaves it there.
 * On a capture too small to fill the chip with blocks of 256 payloads the tiles are spread over gridDim.y (the metadata of 256 payloads
 * is then read once per y block -- a few KiB out of L2).
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "kmpgpu.h"
#include "kmp_device.h"
#include "kmp_launch.h"

namespace {

constexpr uint32_t HDR_THREADS = 256u;
constexpr uint32_t HDR_WAVES = HDR_THREADS / KMP_WAVE;
constexpr uint32_t HDR_REC = 3u;              /* uint4 per predicate record (kmp_rowtables.h, kmp_pack_headers) */
constexpr uint32_t HDR_MAX_BY = 64u;
static_assert(KMP_HDR_TILE * 2u == HDR_THREADS, "the write-out gives every thread 16 bytes of one predicate of the tile");
static_assert(HDR_WAVES == 4u, "a block's words of a row are two 16-byte pieces");

/* a word of a predicate's record: the same in every lane, so into a scalar register, and what is computed from it alone is scalar work */
__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

/* One predicate's record with its ranges as {lo, hi - lo}: lo <= v <= hi is (v - lo) <= (hi - lo) in unsigned arithmetic (lo <= hi is
 * what kmp_pack_headers has checked), one subtraction and one compare per lane. */
struct Pred {
    uint32_t src, src_mask, dst, dst_mask, sport_lo, sport_w, dport_lo, dport_w, len_lo, len_w, proto, any_proto, bidir;
};

/* one direction of a predicate: source and destination as given.  Bitwise, not short-circuit: no branch on a lane's answer */
__device__ __forceinline__ bool dir_holds(const Pred &p, uint32_t s, uint32_t d, uint32_t sp, uint32_t dp)
{
    return ((s & p.src_mask) == p.src) & ((d & p.dst_mask) == p.dst) & ((sp - p.sport_lo) <= p.sport_w) & ((dp - p.dport_lo) <= p.dport_w);
}

__global__ void __launch_bounds__(HDR_THREADS)
kmp_headers_kernel(const uint4 *__restrict__ meta, const uint32_t *__restrict__ pkt_len, uint64_t n_pkts, uint64_t stride,
                   const uint4 *__restrict__ preds, uint32_t n_hdr, ulonglong2 *__restrict__ rows,
                   unsigned long long *__restrict__ hdr_counts, unsigned long long *__restrict__ any)
{
    __shared__ uint4 s_pred[KMP_HDR_TILE * HDR_REC];
    __shared__ ulonglong2 s_out[KMP_HDR_TILE * (HDR_WAVES / 2u)];

    const uint32_t t = threadIdx.x, lane = t & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(t >> 6));
    const uint64_t j = (uint64_t)blockIdx.x * HDR_WAVES + wave;           /* this wavefront's column word */
    const uint64_t k = j * 64u + lane;
    const bool live = k < n_pkts;
    uint4 M = make_uint4(0u, 0u, 0u, 0u);
    uint32_t L = 0u;
    if (live) { M = meta[k]; L = pkt_len[k]; }
    const uint32_t sp = M.z & 0xFFFFu, dp = M.z >> 16, proto = M.w & 0xFFu;

    unsigned long long *s_words = reinterpret_cast<unsigned long long *>(s_out);
    unsigned long long any_acc = 0ull;
    const uint32_t tiles = (n_hdr + KMP_HDR_TILE - 1u) / KMP_HDR_TILE;
    for (uint32_t tile = blockIdx.y; tile < tiles; tile += gridDim.y) {
        const uint32_t q0 = tile * KMP_HDR_TILE;
        const uint32_t nq = min(KMP_HDR_TILE, n_hdr - q0);
        __syncthreads();                                 /* the write-out of the tile before has read s_out */
        for (uint32_t i = t; i < nq * HDR_REC; i += HDR_THREADS) s_pred[i] = preds[(uint64_t)q0 * HDR_REC + i];
        __syncthreads();
        for (uint32_t q = 0; q < nq; ++q) {
            const uint4 a = s_pred[q * HDR_REC];         /* src_ip & src_mask, src_mask, dst_ip & dst_mask, dst_mask */
            const uint4 b = s_pred[q * HDR_REC + 1u];    /* sport_lo | sport_hi << 16, dport_lo | dport_hi << 16, len_lo, len_hi */
            const uint32_t pf = uni(s_pred[q * HDR_REC + 2u].x);     /* proto | flags << 8 */
            const uint32_t sports = uni(b.x), dports = uni(b.y), len_lo = uni(b.z);
            const Pred p = {uni(a.x), uni(a.y), uni(a.z), uni(a.w), sports & 0xFFFFu, (sports >> 16) - (sports & 0xFFFFu), dports & 0xFFFFu,
                            (dports >> 16) - (dports & 0xFFFFu), len_lo, uni(b.w) - len_lo, pf & 0xFFu,
                            (pf >> 8) & KMPGPU_HDR_ANY_PROTO, (pf >> 8) & KMPGPU_HDR_BIDIR};
            const bool ok = live & ((p.any_proto != 0u) | (proto == p.proto)) & ((L - p.len_lo) <= p.len_w);
            const bool fwd = dir_holds(p, M.x, M.y, sp, dp), rev = dir_holds(p, M.y, M.x, dp, sp);
            const bool hit = ok & (fwd | ((p.bidir != 0u) & rev));
            const unsigned long long w = __ballot(hit);
            any_acc |= w;
            if (lane == 0u) s_words[q * HDR_WAVES + wave] = w;
        }
        __syncthreads();
        /* 16 bytes of predicate t / 2 per thread: words 4 blockIdx.x + 2 half and the one behind it (stride is even) */
        const uint32_t q = t >> 1, half = t & 1u;
        const uint64_t col = (uint64_t)blockIdx.x * HDR_WAVES + 2u * half;
        uint32_t pc = 0u;
        if (q < nq && col < stride) {
            const ulonglong2 v = s_out[q * (HDR_WAVES / 2u) + half];
            rows[((uint64_t)(q0 + q) * stride + col) >> 1] = v;
            pc = (uint32_t)__builtin_popcountll(v.x) + (uint32_t)__builtin_popcountll(v.y);
        }
        pc += (uint32_t)__shfl_xor((int)pc, 1);
        if (half == 0u && pc != 0u) atomicAdd(hdr_counts + q0 + q, (unsigned long long)pc);     /* (pc != 0: q < nq) */
    }
    if (lane == 0u && any_acc != 0ull) atomicOr(any + j, any_acc);       /* (a set bit: j < W) */
}

/* The scan workspace (kmp_compact_ws, kmp_launch.h) after its scan.  len[i] == 0xFFFFFFFF: frame (or payload) i was rejected (not selected); otherwise it is payload
 * blk_cnt[i / KMP_SCAN_TILE] + loc_idx[i] of the new arena, as kmp_scatter_index_kernel and kmp_select_index_kernel number them. */

/* KMPGPU_OPT_KEEP_META: the record of every accepted frame, from the byte positions the extractors walk (kmpgpu.h).  For a frame
 * kmp_extract_kernel accepts they all lie inside its captured bytes: udp cl >= 34 and cl - 14 - ihl >= 8, tcp ihl >= 20 and
 * cl >= 14 + ihl + 20. */
__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_meta_extract_kernel(const uint8_t *__restrict__ file, const uint64_t *__restrict__ frame_off, const uint32_t *__restrict__ plen,
                        const uint32_t *__restrict__ loc_idx, const uint32_t *__restrict__ blk_cnt, uint64_t n, uint4 *__restrict__ meta)
{
    for (uint64_t f = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; f < n; f += (uint64_t)gridDim.x * blockDim.x) {
        if (plen[f] == 0xFFFFFFFFu) continue;
        const uint64_t k = (uint64_t)blk_cnt[f / KMP_SCAN_TILE] + loc_idx[f];
        const uint8_t *p = file + frame_off[f];
        const uint32_t at = 14u + ((uint32_t)(p[14] & 0x0Fu) << 2);
        const uint32_t src = (uint32_t)p[26] << 24 | (uint32_t)p[27] << 16 | (uint32_t)p[28] << 8 | p[29];
        const uint32_t dst = (uint32_t)p[30] << 24 | (uint32_t)p[31] << 16 | (uint32_t)p[32] << 8 | p[33];
        const uint32_t sport = (uint32_t)p[at] << 8 | p[at + 1u], dport = (uint32_t)p[at + 2u] << 8 | p[at + 3u];
        meta[k] = make_uint4(src, dst, sport | dport << 16, p[23]);
    }
}

/* kmpgpu_load_selected: the records of the selected payloads, in their new order */
__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_meta_select_kernel(const uint4 *__restrict__ src_meta, const uint32_t *__restrict__ sel_len, const uint32_t *__restrict__ loc_idx,
                       const uint32_t *__restrict__ blk_cnt, uint64_t n, uint4 *__restrict__ meta)
{
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (uint64_t)gridDim.x * blockDim.x) {
        if (sel_len[k] == 0xFFFFFFFFu) continue;
        meta[(uint64_t)blk_cnt[k / KMP_SCAN_TILE] + loc_idx[k]] = src_meta[k];
    }
}

}  // namespace

hipError_t kmp_launch_headers(const void *meta, const uint32_t *pkt_len, uint64_t n_pkts, uint64_t stride, const uint4 *preds,
                              uint32_t n_hdr, unsigned long long *rows, unsigned long long *hdr_counts, unsigned long long *any,
                              hipStream_t st)
{
    static_assert(sizeof(kmpgpu_pkt_meta) == sizeof(uint4), "a metadata record is one 16-byte load");
    if (n_hdr == 0 || n_pkts == 0) return hipSuccess;
    if ((stride & 1u) || n_pkts > stride * 64u) return hipErrorInvalidValue;
    const uint64_t bx = (stride + HDR_WAVES - 1u) / HDR_WAVES;
    if (bx > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const uint32_t tiles = (n_hdr + KMP_HDR_TILE - 1u) / KMP_HDR_TILE;
    const uint32_t by = (uint32_t)std::min<uint64_t>(std::min(tiles, HDR_MAX_BY), std::max<uint64_t>(1u, 1024u / bx));
    hipLaunchKernelGGL(kmp_headers_kernel, dim3((uint32_t)bx, by), dim3(HDR_THREADS), 0, st, reinterpret_cast<const uint4 *>(meta), pkt_len,
                       n_pkts, stride, preds, n_hdr, reinterpret_cast<ulonglong2 *>(rows), hdr_counts, any);
    return hipGetLastError();
}

hipError_t kmp_launch_meta_extract(const uint8_t *file, const uint64_t *frame_off, uint64_t n, const uint8_t *ws, void *meta, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    const kmp_compact_view w = kmp_compact_ws(const_cast<uint8_t *>(ws), n);
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((n + KMP_BLOCK_THREADS - 1) / KMP_BLOCK_THREADS, 4096);
    hipLaunchKernelGGL(kmp_meta_extract_kernel, dim3(blocks), dim3(KMP_BLOCK_THREADS), 0, st, file, frame_off, w.len, w.loc_idx, w.blk_cnt, n,
                       reinterpret_cast<uint4 *>(meta));
    return hipGetLastError();
}

hipError_t kmp_launch_meta_select(const void *src_meta, uint64_t n, const uint8_t *ws, void *meta, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    const kmp_compact_view w = kmp_compact_ws(const_cast<uint8_t *>(ws), n);
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((n + KMP_BLOCK_THREADS - 1) / KMP_BLOCK_THREADS, 1024);
    hipLaunchKernelGGL(kmp_meta_select_kernel, dim3(blocks), dim3(KMP_BLOCK_THREADS), 0, st, reinterpret_cast<const uint4 *>(src_meta), w.len,
                       w.loc_idx, w.blk_cnt, n, reinterpret_cast<uint4 *>(meta));
    return hipGetLastError();
}
