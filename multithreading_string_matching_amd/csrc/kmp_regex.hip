/*
 * kmp_regex.hip -- the expressions of kmpgpu_scan_regexes / kmpgpu_scan_rules on gfx950 (kmpgpu_set_regexes, kmpgpu.h): byte classes and
 * repeats compiled on the host into position automata of at most 63 positions (kmp_regex.h), stepped here once per text byte.  The kernel
 * runs behind the marking pass and writes one further row of the hit matrix per expression, its own rows only:
 *   rows[q][j]    = for the payloads k of word j: expression q matches in payload k, and payload k holds q's gate pattern where it has one
 *   rx_counts[q]  = the set bits of row q
 *   any[j]        = OR over all expressions of word j
 *
 * The shape of kmp_bytetests_abs_kernel and kmp_headers_kernel: a lane owns a payload, a wavefront owns a column word, a block of four
 * wavefronts owns four consecutive words.  The expressions come in tiles of KMP_RX_TILE out of LDS (kmp_regex.h: per tile B[256][tile] as
 * 64-bit words and a 32-byte record per expression).  A lane keeps one 64-bit reach set R per expression of the tile in registers -- bit i:
 * position i is next, bit n: accepted -- and walks its payload in aligned 16-byte loads from pkt_off[k] on, none at or behind
 * round_up(L_k, 16).  Per text byte c it reads the tile's words of c, 16 bytes at a time, and steps every expression:
 *     b = R & B[c];  N = b << 1 | b & REP | restart;  R = N | ((OPT + (N & OPT)) ^ OPT)
 * The last term is closure(N), every position reachable by passing over optional ones, in one step: adding the optional positions of N to
 * OPT carries through each run of optional positions up to the first position behind it.  An expression without $ is accepted for good
 * once it is: the host set bit n in its B words and in REP.  One with $ is decided by R behind the text's last byte.
 * kmp_regex_kernel<false> ends a lane's text at the first 0x00 it steps onto, kmp_regex_kernel<true> at L_k.  A lane is done with an
 * expression once it has accepted (no $) or its text has ended, and idle for one whose gate bit it lacks; the wavefront leaves the byte
 * loop when every lane is done with every expression of the tile, and skips the walk where no lane holds any gate of the tile.
 * Stores, counts and any[] as in kmp_bytetests.hip: 16-byte pieces of a row through LDS, one atomicAdd per (block, row), one atomicOr per
 * wavefront.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "kmpgpu.h"
#include "kmp_device.h"
#include "kmp_launch.h"
#include "kmp_regex.h"                    /* KMP_RX_TILE and the layout of a tile of the table */
#include "kmp_sweep_dev.h"                /* first_nul16 */

namespace {

constexpr uint32_t RX_THREADS = 256u;
constexpr uint32_t RX_WAVES = RX_THREADS / KMP_WAVE;
constexpr uint32_t RX_MAX_BY = 64u;
constexpr uint32_t RX_TILE_QUADS = KMP_RX_TILE_WORDS / 4u;        /* uint4 per tile of the table */
constexpr uint32_t RX_B_QUADS = 128u * KMP_RX_TILE;               /* ... of which the B words */
static_assert(KMP_RX_TILE % 2u == 0u && KMP_RX_TILE * 2u <= RX_THREADS, "the write-out gives a thread 16 bytes of one expression of the tile");
static_assert(RX_WAVES == 4u, "a block's words of a row are two 16-byte pieces");

__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

/* every position reachable from N by passing over optional ones (see the top of the file) */
__device__ __forceinline__ uint64_t closure(uint64_t N, uint64_t opt) { return N | ((opt + (N & opt)) ^ opt); }

template <bool WHOLE>
__global__ void __launch_bounds__(RX_THREADS)
kmp_regex_kernel(const uint8_t *__restrict__ arena, const uint64_t *__restrict__ pkt_off, const uint32_t *__restrict__ pkt_len,
                 uint64_t n_pkts, uint64_t stride, const unsigned long long *__restrict__ marks, const uint4 *__restrict__ tables,
                 uint32_t n_rx, ulonglong2 *__restrict__ rows, unsigned long long *__restrict__ rx_counts,
                 unsigned long long *__restrict__ any)
{
    __shared__ ulonglong2 s_B[RX_B_QUADS];                               /* [256][KMP_RX_TILE] 64-bit words */
    __shared__ uint4 s_rec[KMP_RX_TILE * 2u];
    __shared__ ulonglong2 s_out[KMP_RX_TILE * (RX_WAVES / 2u)];

    const uint32_t t = threadIdx.x, lane = t & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(t >> 6));
    const uint64_t j = (uint64_t)blockIdx.x * RX_WAVES + wave;            /* this wavefront's column word */
    const uint64_t k = j * 64u + lane;
    const bool valid = k < n_pkts;
    const uint8_t *text = arena;
    uint32_t L = 0u;
    if (valid) { text = arena + pkt_off[k]; L = pkt_len[k]; }

    unsigned long long *s_words = reinterpret_cast<unsigned long long *>(s_out);
    unsigned long long any_acc = 0ull;
    const uint32_t tiles = (n_rx + KMP_RX_TILE - 1u) / KMP_RX_TILE;
    for (uint32_t tile = blockIdx.y; tile < tiles; tile += gridDim.y) {
        const uint32_t q0 = tile * KMP_RX_TILE;
        const uint32_t nq = min(KMP_RX_TILE, n_rx - q0);
        __syncthreads();                                 /* the write-out of the tile before has read s_out and s_rec */
        {
            const uint4 *src = tables + (uint64_t)tile * RX_TILE_QUADS;
            uint4 *dst = reinterpret_cast<uint4 *>(s_B);
            for (uint32_t i = t; i < RX_B_QUADS; i += RX_THREADS) dst[i] = src[i];
            if (t < KMP_RX_TILE * 2u) s_rec[t] = src[RX_B_QUADS + t];
        }
        __syncthreads();

        /* the tile's records, wavefront-uniform; which expressions this lane looks at */
        uint64_t OPT[KMP_RX_TILE], REP[KMP_RX_TILE], R[KMP_RX_TILE];
        uint32_t NPOS[KMP_RX_TILE], RESTART[KMP_RX_TILE];
        uint32_t act = 0u, noeol = 0u;
#pragma unroll
        for (uint32_t q = 0; q < KMP_RX_TILE; ++q) {
            const uint4 a = s_rec[q * 2u], b = s_rec[q * 2u + 1u];
            OPT[q] = (uint64_t)uni(a.y) << 32 | uni(a.x);
            REP[q] = (uint64_t)uni(a.w) << 32 | uni(a.z);
            const uint32_t meta = uni(b.x), gate = uni(b.y);
            NPOS[q] = meta & 0xFFu;
            RESTART[q] = (meta >> 8) & 1u;
            if (!((meta >> 10) & 1u)) noeol |= 1u << q;
            unsigned long long gw = ~0ull;
            if ((meta >> 9) & 1u) gw = j < stride ? marks[(uint64_t)gate * stride + j] : 0ull;       /* (wavefront-uniform) */
            if (q < nq && valid && ((gw >> lane) & 1ull)) act |= 1u << q;
            R[q] = closure(1ull, OPT[q]);
        }

        if (__ballot(act != 0u) != 0ull) {
            uint32_t p = 0u;
            bool ended = L == 0u || act == 0u;
            for (;;) {
                /* done with an expression: accepted and no $ to wait for */
                uint32_t accepted = 0u;
#pragma unroll
                for (uint32_t q = 0; q < KMP_RX_TILE; ++q) accepted |= (uint32_t)((R[q] >> NPOS[q]) & 1ull) << q;
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
                        const ulonglong2 *row = s_B + c * (KMP_RX_TILE / 2u);
#pragma unroll
                        for (uint32_t h = 0; h < KMP_RX_TILE / 2u; ++h) {
                            if (2u * h >= nq) break;                                      /* (wavefront-uniform) the last tile's empty slots */
                            const ulonglong2 bw = row[h];
                            const uint64_t b0 = R[2u * h] & bw.x, b1 = R[2u * h + 1u] & bw.y;
                            R[2u * h] = closure(b0 << 1 | (b0 & REP[2u * h]) | RESTART[2u * h], OPT[2u * h]);
                            R[2u * h + 1u] = closure(b1 << 1 | (b1 & REP[2u * h + 1u]) | RESTART[2u * h + 1u], OPT[2u * h + 1u]);
                        }
                    }
                }
            }
        }
#pragma unroll
        for (uint32_t q = 0; q < KMP_RX_TILE; ++q) {
            const unsigned long long w = __ballot(((act >> q) & 1u) != 0u && ((R[q] >> NPOS[q]) & 1ull) != 0ull);
            any_acc |= w;
            if (lane == 0u) s_words[q * RX_WAVES + wave] = w;
        }
        __syncthreads();
        /* 16 bytes of expression t / 2 per thread: words 4 blockIdx.x + 2 half and the one behind it (stride is even) */
        const uint32_t q = t >> 1, half = t & 1u;
        const uint64_t col = (uint64_t)blockIdx.x * RX_WAVES + 2u * half;
        uint32_t pc = 0u;
        if (q < nq && col < stride) {
            const ulonglong2 v = s_out[q * (RX_WAVES / 2u) + half];
            rows[((uint64_t)(q0 + q) * stride + col) >> 1] = v;
            pc = (uint32_t)__builtin_popcountll(v.x) + (uint32_t)__builtin_popcountll(v.y);
        }
        pc += (uint32_t)__shfl_xor((int)pc, 1);
        if (half == 0u && pc != 0u) atomicAdd(rx_counts + q0 + q, (unsigned long long)pc);      /* (pc != 0: q < nq) */
    }
    if (lane == 0u && any_acc != 0ull) atomicOr(any + j, any_acc);       /* (a set bit: j < W) */
}

}  // namespace

hipError_t kmp_launch_regexes(const unsigned long long *marks, uint64_t stride, uint64_t n_pkts, const uint4 *tables, uint32_t n_rx,
                              const uint8_t *arena, const uint64_t *pkt_off, const uint32_t *pkt_len, bool whole,
                              unsigned long long *rows, unsigned long long *rx_counts, unsigned long long *any, hipStream_t st)
{
    const uint64_t W = (n_pkts + 63u) / 64u;
    if (n_rx == 0 || W == 0) return hipSuccess;
    if ((stride & 1u) || W > stride) return hipErrorInvalidValue;
    const uint64_t bx = (stride + RX_WAVES - 1u) / RX_WAVES;
    if (bx > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const uint32_t tiles = (n_rx + KMP_RX_TILE - 1u) / KMP_RX_TILE;
    const uint32_t by = (uint32_t)std::min<uint64_t>(std::min(tiles, RX_MAX_BY), std::max<uint64_t>(1u, 1024u / bx));
    const dim3 grid((uint32_t)bx, by);
    if (whole)
        hipLaunchKernelGGL(kmp_regex_kernel<true>, grid, dim3(RX_THREADS), 0, st, arena, pkt_off, pkt_len, n_pkts, stride, marks, tables, n_rx,
                           reinterpret_cast<ulonglong2 *>(rows), rx_counts, any);
    else
        hipLaunchKernelGGL(kmp_regex_kernel<false>, grid, dim3(RX_THREADS), 0, st, arena, pkt_off, pkt_len, n_pkts, stride, marks, tables, n_rx,
                           reinterpret_cast<ulonglong2 *>(rows), rx_counts, any);
    return hipGetLastError();
}
