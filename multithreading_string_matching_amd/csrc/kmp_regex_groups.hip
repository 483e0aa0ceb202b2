/*
 * kmp_regex_groups.hip -- the expressions under KMPGPU_RX_GROUPS on gfx950 (kmpgpu_set_regexes, kmpgpu.h): groups and alternation, compiled
 * on the host into Glushkov position automata of at most 63 positions and KMPGPU_RX_MAX_EDGES edge rules (kmp_regex.h), stepped here once
 * per text byte.  The kernel runs behind kmp_regex_kernel and writes the rows of the flagged expressions, each at the index q its record
 * carries; counts and any[] as there.
 *
 * The shape of kmp_regex_kernel: a lane owns a payload, a wavefront owns a column word, a block of four wavefronts owns four consecutive
 * words; the expressions come in tiles of KMP_RXG_TILE out of LDS (kmp_regex.h: per tile B[256][tile] as 64-bit words, a 48-byte record
 * and KMPGPU_RX_MAX_EDGES 16-byte rules per expression).  A lane keeps one 64-bit reach set R per expression of the tile in registers and
 * walks its payload in aligned 16-byte loads from pkt_off[k] on, none at or behind round_up(L_k, 16).  Per text byte c:
 *     b = R & B[c];  N = (b & SHIFT) << 1 | b & REP | OR over the rules r with (b & src[r]) != 0 of dst[r];
 *     R = N | ((OPT + (N & OPT)) ^ OPT) | restart
 * restart: FIRST where there is no leading ^.  The masks are wavefront-uniform and live in SGPRs; the rules are read from LDS at one
 * address per wavefront, a uniform number of them per expression.  Everything else -- the sticky accept bit, $, the text-end rules, the
 * gates, when a lane and a wavefront are done, the stores through LDS -- is kmp_regex_kernel's.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "kmpgpu.h"
#include "kmp_device.h"
#include "kmp_launch.h"
#include "kmp_regex.h"                    /* KMP_RXG_TILE and the layout of a tile of the table */
#include "kmp_sweep_dev.h"                /* first_nul16 */

namespace {

constexpr uint32_t RXG_THREADS = 256u;
constexpr uint32_t RXG_WAVES = RXG_THREADS / KMP_WAVE;
constexpr uint32_t RXG_MAX_BY = 64u;
constexpr uint32_t RXG_TILE_QUADS = KMP_RXG_TILE_WORDS / 4u;      /* uint4 per tile of the table */
constexpr uint32_t RXG_B_QUADS = 128u * KMP_RXG_TILE;             /* ... of which the B words */
constexpr uint32_t RXG_REC_QUADS = 3u * KMP_RXG_TILE;             /* ... the records */
constexpr uint32_t RXG_RULE_QUADS = KMPGPU_RX_MAX_EDGES * KMP_RXG_TILE;
static_assert(RXG_TILE_QUADS == RXG_B_QUADS + RXG_REC_QUADS + RXG_RULE_QUADS, "a tile is B words, records and rules");
static_assert(KMP_RXG_TILE % 2u == 0u && KMP_RXG_TILE * 2u <= RXG_THREADS, "the write-out gives a thread 16 bytes of one expression of the tile");
static_assert(RXG_REC_QUADS + RXG_RULE_QUADS <= RXG_THREADS, "one thread per 16 bytes of records and rules");
static_assert(RXG_WAVES == 4u, "a block's words of a row are two 16-byte pieces");

__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint64_t uni64(uint32_t lo, uint32_t hi) { return (uint64_t)uni(hi) << 32 | uni(lo); }

__device__ __forceinline__ uint64_t closure(uint64_t N, uint64_t opt) { return N | ((opt + (N & opt)) ^ opt); }

template <bool WHOLE>
__global__ void __launch_bounds__(RXG_THREADS)
kmp_regex_groups_kernel(const uint8_t *__restrict__ arena, const uint64_t *__restrict__ pkt_off, const uint32_t *__restrict__ pkt_len,
                        uint64_t n_pkts, uint64_t stride, const unsigned long long *__restrict__ marks, const uint4 *__restrict__ tables,
                        uint32_t n_groups, ulonglong2 *__restrict__ rows, unsigned long long *__restrict__ rx_counts,
                        unsigned long long *__restrict__ any)
{
    __shared__ ulonglong2 s_B[RXG_B_QUADS];                              /* [256][KMP_RXG_TILE] 64-bit words */
    __shared__ uint4 s_rec[RXG_REC_QUADS];
    __shared__ ulonglong2 s_rule[RXG_RULE_QUADS];                        /* [KMP_RXG_TILE][KMPGPU_RX_MAX_EDGES] {src, dst} */
    __shared__ ulonglong2 s_out[KMP_RXG_TILE * (RXG_WAVES / 2u)];

    const uint32_t t = threadIdx.x, lane = t & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(t >> 6));
    const uint64_t j = (uint64_t)blockIdx.x * RXG_WAVES + wave;           /* this wavefront's column word */
    const uint64_t k = j * 64u + lane;
    const bool valid = k < n_pkts;
    const uint8_t *text = arena;
    uint32_t L = 0u;
    if (valid) { text = arena + pkt_off[k]; L = pkt_len[k]; }

    unsigned long long *s_words = reinterpret_cast<unsigned long long *>(s_out);
    unsigned long long any_acc = 0ull;
    const uint32_t tiles = (n_groups + KMP_RXG_TILE - 1u) / KMP_RXG_TILE;
    for (uint32_t tile = blockIdx.y; tile < tiles; tile += gridDim.y) {
        const uint32_t nq = min(KMP_RXG_TILE, n_groups - tile * KMP_RXG_TILE);
        __syncthreads();                                 /* the write-out of the tile before has read s_out and s_rec */
        {
            const uint4 *src = tables + (uint64_t)tile * RXG_TILE_QUADS;
            uint4 *dst = reinterpret_cast<uint4 *>(s_B);
            for (uint32_t i = t; i < RXG_B_QUADS; i += RXG_THREADS) dst[i] = src[i];
            if (t < RXG_REC_QUADS) s_rec[t] = src[RXG_B_QUADS + t];
            else if (t < RXG_REC_QUADS + RXG_RULE_QUADS)
                reinterpret_cast<uint4 *>(s_rule)[t - RXG_REC_QUADS] = src[RXG_B_QUADS + t];
        }
        __syncthreads();

        /* the tile's records, wavefront-uniform; which expressions this lane looks at */
        uint64_t OPT[KMP_RXG_TILE], REP[KMP_RXG_TILE], SHIFT[KMP_RXG_TILE], RESTART[KMP_RXG_TILE], R[KMP_RXG_TILE];
        uint32_t NPOS[KMP_RXG_TILE], NRULES[KMP_RXG_TILE];
        uint32_t act = 0u, noeol = 0u;
#pragma unroll
        for (uint32_t q = 0; q < KMP_RXG_TILE; ++q) {
            const uint4 a = s_rec[q * 3u], b = s_rec[q * 3u + 1u], c = s_rec[q * 3u + 2u];
            OPT[q] = uni64(a.x, a.y);
            REP[q] = uni64(a.z, a.w);
            SHIFT[q] = uni64(b.x, b.y);
            const uint64_t first = uni64(b.z, b.w);
            const uint32_t meta = uni(c.x), gate = uni(c.y);
            NPOS[q] = meta & 0xFFu;
            NRULES[q] = min(meta >> 16, (uint32_t)KMPGPU_RX_MAX_EDGES);
            RESTART[q] = ((meta >> 8) & 1u) ? first : 0ull;
            if (!((meta >> 10) & 1u)) noeol |= 1u << q;
            unsigned long long gw = ~0ull;
            if ((meta >> 9) & 1u) gw = j < stride ? marks[(uint64_t)gate * stride + j] : 0ull;       /* (wavefront-uniform) */
            if (q < nq && valid && ((gw >> lane) & 1ull)) act |= 1u << q;
            R[q] = first;
        }

        if (__ballot(act != 0u) != 0ull) {
            uint32_t p = 0u;
            bool ended = L == 0u || act == 0u;
            for (;;) {
                /* done with an expression: accepted and no $ to wait for */
                uint32_t accepted = 0u;
#pragma unroll
                for (uint32_t q = 0; q < KMP_RXG_TILE; ++q) accepted |= (uint32_t)((R[q] >> NPOS[q]) & 1ull) << q;
                const bool go = !ended && (act & ~(accepted & noeol)) != 0u;
                if (__ballot(go) == 0ull) break;
                if (go) {
                    uint4 v = *reinterpret_cast<const uint4 *>(text + p);             /* p < L: inside the payload's 16-byte-rounded slot */
                    uint32_t nv = min(16u, L - p);
                    if (!WHOLE) nv = min(nv, first_nul16(v));
                    p += 16u;
                    ended = nv < 16u || p >= L;
                    for (uint32_t i = 0; i < nv; ++i) {
                        const uint32_t c = v.x & 0xFFu;
                        v.x = __builtin_amdgcn_alignbit(v.y, v.x, 8u);
                        v.y = __builtin_amdgcn_alignbit(v.z, v.y, 8u);
                        v.z = __builtin_amdgcn_alignbit(v.w, v.z, 8u);
                        v.w >>= 8;
                        const ulonglong2 *row = s_B + c * (KMP_RXG_TILE / 2u);
#pragma unroll
                        for (uint32_t h = 0; h < KMP_RXG_TILE / 2u; ++h) {
                            if (2u * h >= nq) break;                                      /* (wavefront-uniform) the last tile's empty slots */
                            const ulonglong2 bw = row[h];
#pragma unroll
                            for (uint32_t e = 0; e < 2u; ++e) {
                                const uint32_t q = 2u * h + e;
                                const uint64_t b = R[q] & (e ? bw.y : bw.x);
                                uint64_t N = (b & SHIFT[q]) << 1 | (b & REP[q]);
                                for (uint32_t r = 0; r < NRULES[q]; ++r) {                  /* (a uniform trip count, one LDS address per wavefront) */
                                    const ulonglong2 rule = s_rule[q * KMPGPU_RX_MAX_EDGES + r];
                                    if ((b & rule.x) != 0ull) N |= rule.y;
                                }
                                R[q] = closure(N, OPT[q]) | RESTART[q];
                            }
                        }
                    }
                }
            }
        }
#pragma unroll
        for (uint32_t q = 0; q < KMP_RXG_TILE; ++q) {
            const unsigned long long w = __ballot(((act >> q) & 1u) != 0u && ((R[q] >> NPOS[q]) & 1ull) != 0ull);
            any_acc |= w;
            if (lane == 0u) s_words[q * RXG_WAVES + wave] = w;
        }
        __syncthreads();
        /* 16 bytes of expression t / 2 per thread, to the row its record names: words 4 blockIdx.x + 2 half and the one behind it */
        const uint32_t q = t >> 1, half = t & 1u;
        const uint64_t col = (uint64_t)blockIdx.x * RXG_WAVES + 2u * half;
        uint32_t pc = 0u, row_q = 0u;
        if (q < nq && col < stride) {
            row_q = s_rec[q * 3u + 2u].z;
            const ulonglong2 v = s_out[q * (RXG_WAVES / 2u) + half];
            rows[((uint64_t)row_q * stride + col) >> 1] = v;
            pc = (uint32_t)__builtin_popcountll(v.x) + (uint32_t)__builtin_popcountll(v.y);
        }
        pc += (uint32_t)__shfl_xor((int)pc, 1);
        if (half == 0u && pc != 0u) atomicAdd(rx_counts + row_q, (unsigned long long)pc);       /* (pc != 0: q < nq) */
    }
    if (lane == 0u && any_acc != 0ull) atomicOr(any + j, any_acc);       /* (a set bit: j < W) */
}

}  // namespace

hipError_t kmp_launch_regex_groups(const unsigned long long *marks, uint64_t stride, uint64_t n_pkts, const uint4 *tables, uint32_t n_groups,
                                   const uint8_t *arena, const uint64_t *pkt_off, const uint32_t *pkt_len, bool whole,
                                   unsigned long long *rows, unsigned long long *rx_counts, unsigned long long *any, hipStream_t st)
{
    const uint64_t W = (n_pkts + 63u) / 64u;
    if (n_groups == 0 || W == 0) return hipSuccess;
    if ((stride & 1u) || W > stride) return hipErrorInvalidValue;
    const uint64_t bx = (stride + RXG_WAVES - 1u) / RXG_WAVES;
    if (bx > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const uint32_t tiles = (n_groups + KMP_RXG_TILE - 1u) / KMP_RXG_TILE;
    const uint32_t by = (uint32_t)std::min<uint64_t>(std::min(tiles, RXG_MAX_BY), std::max<uint64_t>(1u, 1024u / bx));
    const dim3 grid((uint32_t)bx, by);
    if (whole)
        hipLaunchKernelGGL(kmp_regex_groups_kernel<true>, grid, dim3(RXG_THREADS), 0, st, arena, pkt_off, pkt_len, n_pkts, stride, marks, tables,
                           n_groups, reinterpret_cast<ulonglong2 *>(rows), rx_counts, any);
    else
        hipLaunchKernelGGL(kmp_regex_groups_kernel<false>, grid, dim3(RXG_THREADS), 0, st, arena, pkt_off, pkt_len, n_pkts, stride, marks, tables,
                           n_groups, reinterpret_cast<ulonglong2 *>(rows), rx_counts, any);
    return hipGetLastError();
}
