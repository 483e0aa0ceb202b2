/*
 * kmp_bytetests.hip -- the byte tests of kmpgpu_scan_bytetests / kmpgpu_scan_rules on gfx950 (kmpgpu_set_bytetests, kmpgpu.h): 1 to 4 bytes
 * of a payload taken as an unsigned integer in either byte order, masked and compared.  Both kernels run behind the marking pass and write
 * one further row of the hit matrix per test, each kernel its own rows only:
 *   rows[q][j]    = for the payloads k of word j: test q holds for payload k
 *   bt_counts[q]  = the set bits of row q
 *   any[j]        = OR over all tests of word j
 * The record of test q is two uint4 (kmp_rowtables.h, kmp_pack_bytetests): {anchor | fold << 31, offset, mask, value} and
 * {nbytes | op << 8 | flags << 16, 0, 0, 0}.
 *
 * Absolute tests (kmp_bytetests_abs_kernel), the shape of kmp_headers_kernel: a lane owns a payload, a wavefront owns a column word, a block
 * of four wavefronts owns four consecutive words.  A lane loads its payload's offset and length once and, under the strlen rule, looks for
 * the first 0x00 among the first min(L_k, H) bytes in 16-byte loads, leaving at the first one found (H: the largest offset + nbytes of the
 * absolute tests -- no test reads behind it, so a text that ends behind H ends "late enough" wherever it does).  The tests come in tiles
 * of KMP_BT_TILE out of LDS, their records wavefront-uniform: per test a lane whose field lies inside the text loads the aligned dword
 * that holds the field's first byte and, only where the field crosses into the next dword, that one too.  Both hold a byte of the field,
 * a byte in front of E_k <= L_k: nothing outside the payload's 16-byte-rounded slot is read.  The field in either byte order, the mask and
 * the compare are straight-line code; 64 answers make the row word with one ballot.  Stores, counts and any[] as in kmp_headers.hip:
 * 16-byte pieces of a row through LDS, one atomicAdd per (block, row), one atomicOr per wavefront.  The relative tests of a tile are
 * passed over, and their rows are not written.
 *
 * Relative tests (kmp_bytetests_rel_kernel), the shape of kmp_relations_kernel: one wavefront per (relative test, word j), grid-stride.
 * Candidates are the payloads that hold the anchor, marks[anchor][j].  Per candidate one ascending sweep, a lane per start offset x of
 * the anchor, 64 per step, over the only starts that can serve: x >= 0, inside the window, and the field x + m + offset .. + nbytes
 * inside [0, E_k).  The lanes whose x matches (kmp_sweep_dev.h: in the fold where the anchor is a nocase pattern) read their field byte
 * by byte from the ORIGINAL arena and compare; the first step with a success ends the sweep.  No memory grows with the payload.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "kmpgpu.h"
#include "kmp_device.h"
#include "kmp_launch.h"
#include "kmp_sweep_dev.h"                /* first_nul16, text_end, match_at */

namespace {

constexpr uint32_t BT_THREADS = 256u;
constexpr uint32_t BT_WAVES = BT_THREADS / KMP_WAVE;
constexpr uint32_t BT_REC = 2u;               /* uint4 per test record */
constexpr uint32_t BT_MAX_BY = 64u;
static_assert(KMP_BT_TILE * 2u == BT_THREADS, "the write-out gives every thread 16 bytes of one test of the tile");
static_assert(BT_WAVES == 4u, "a block's words of a row are two 16-byte pieces");

__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

/* which of (field < value, field == value, field > value) satisfy op: bits 0, 1, 2 of the op's three bits */
constexpr uint32_t BT_OP_BITS = 2u << (3 * KMPGPU_BT_EQ) | 5u << (3 * KMPGPU_BT_NE) | 1u << (3 * KMPGPU_BT_LT) | 4u << (3 * KMPGPU_BT_GT) |
                                3u << (3 * KMPGPU_BT_LE) | 6u << (3 * KMPGPU_BT_GE);

/* ((field & mask) op value), unsigned; want: the op's three bits.  No branch */
__device__ __forceinline__ bool compare(uint32_t field, uint32_t mask, uint32_t value, uint32_t want)
{
    const uint32_t x = field & mask;
    return (((x < value) & (want & 1u)) | ((x == value) & ((want >> 1) & 1u)) | ((x > value) & (want >> 2))) != 0u;
}

template <bool WHOLE>
__global__ void __launch_bounds__(BT_THREADS)
kmp_bytetests_abs_kernel(const uint8_t *__restrict__ arena, const uint64_t *__restrict__ pkt_off, const uint32_t *__restrict__ pkt_len,
                         uint64_t n_pkts, uint64_t stride, const uint4 *__restrict__ tests, uint32_t n_bt, uint32_t H,
                         ulonglong2 *__restrict__ rows, unsigned long long *__restrict__ bt_counts, unsigned long long *__restrict__ any)
{
    __shared__ uint4 s_rec[KMP_BT_TILE * BT_REC];
    __shared__ ulonglong2 s_out[KMP_BT_TILE * (BT_WAVES / 2u)];

    const uint32_t t = threadIdx.x, lane = t & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(t >> 6));
    const uint64_t j = (uint64_t)blockIdx.x * BT_WAVES + wave;            /* this wavefront's column word */
    const uint64_t k = j * 64u + lane;
    const uint8_t *text = arena;
    uint32_t E = 0u;                                                      /* a lane at n_pkts or behind: no field is defined */
    if (k < n_pkts) { text = arena + pkt_off[k]; E = pkt_len[k]; }
    if (!WHOLE) {
        const uint32_t lim = min(E, H);
        for (uint32_t p = 0; p < lim; p += 16u) {
            const uint32_t z = first_nul16(*reinterpret_cast<const uint4 *>(text + p));
            if (z < 16u) { E = min(E, p + z); break; }
        }
    }

    unsigned long long *s_words = reinterpret_cast<unsigned long long *>(s_out);
    unsigned long long any_acc = 0ull;
    const uint32_t tiles = (n_bt + KMP_BT_TILE - 1u) / KMP_BT_TILE;
    for (uint32_t tile = blockIdx.y; tile < tiles; tile += gridDim.y) {
        const uint32_t q0 = tile * KMP_BT_TILE;
        const uint32_t nq = min(KMP_BT_TILE, n_bt - q0);
        __syncthreads();                                 /* the write-out of the tile before has read s_out and s_rec */
        for (uint32_t i = t; i < nq * BT_REC; i += BT_THREADS) s_rec[i] = tests[(uint64_t)q0 * BT_REC + i];
        __syncthreads();
        for (uint32_t q = 0; q < nq; ++q) {
            const uint32_t nof = uni(s_rec[q * BT_REC + 1u].x);          /* nbytes | op << 8 | flags << 16 */
            if ((nof >> 16) & KMPGPU_BT_RELATIVE) continue;               /* (wavefront-uniform) the other kernel's row */
            const uint4 a = s_rec[q * BT_REC];
            const uint32_t pos = uni(a.y), mask = uni(a.z), value = uni(a.w);
            const uint32_t nb = nof & 0xFFu, want = (BT_OP_BITS >> (3u * ((nof >> 8) & 0xFFu))) & 7u;
            const uint32_t sh = (pos & 3u) * 8u;
            const bool defined = pos + nb <= E;                          /* (pos <= 2^31 - 1: no wrap) */
            uint32_t w0 = 0u, w1 = 0u;
            if (defined) {
                const uint32_t *p = reinterpret_cast<const uint32_t *>(text + (pos & ~3u));
                w0 = p[0];
                if ((pos & 3u) + nb > 4u) w1 = p[1];                     /* (the condition is the test's alone) */
            }
            const uint32_t raw = (uint32_t)(((uint64_t)w1 << 32 | w0) >> sh);        /* byte pos in the low byte */
            const uint32_t le = raw & (0xFFFFFFFFu >> (32u - 8u * nb));
            const uint32_t be = __builtin_bswap32(raw) >> (32u - 8u * nb);
            const uint32_t field = ((nof >> 16) & KMPGPU_BT_LITTLE) ? le : be;
            const unsigned long long w = __ballot(defined & compare(field, mask, value, want));
            any_acc |= w;
            if (lane == 0u) s_words[q * BT_WAVES + wave] = w;
        }
        __syncthreads();
        /* 16 bytes of test t / 2 per thread: words 4 blockIdx.x + 2 half and the one behind it (stride is even) */
        const uint32_t q = t >> 1, half = t & 1u;
        const uint64_t col = (uint64_t)blockIdx.x * BT_WAVES + 2u * half;
        uint32_t pc = 0u;
        if (q < nq && col < stride && !((s_rec[q * BT_REC + 1u].x >> 16) & KMPGPU_BT_RELATIVE)) {
            const ulonglong2 v = s_out[q * (BT_WAVES / 2u) + half];
            rows[((uint64_t)(q0 + q) * stride + col) >> 1] = v;
            pc = (uint32_t)__builtin_popcountll(v.x) + (uint32_t)__builtin_popcountll(v.y);
        }
        pc += (uint32_t)__shfl_xor((int)pc, 1);
        if (half == 0u && pc != 0u) atomicAdd(bt_counts + q0 + q, (unsigned long long)pc);      /* (pc != 0: q < nq) */
    }
    if (lane == 0u && any_acc != 0ull) atomicOr(any + j, any_acc);       /* (a set bit: j < W) */
}

/* The sweep of one candidate (see the top of the file).  Everything but the lane is wave-uniform, and so is the result. */
__device__ __forceinline__ bool bytetest_holds(const uint8_t *__restrict__ text_a, const uint8_t *__restrict__ text,
                                               const kmp_pattern_dev *__restrict__ pa, int32_t offset, uint32_t nb, bool little,
                                               uint32_t mask, uint32_t value, uint32_t want, uint32_t E32, uint2 win, uint32_t lane)
{
    const long long E = E32, m = pa->m, rel = m + (long long)offset;      /* field position = x + rel */
    long long x_first = (long long)win.x > -rel ? (long long)win.x : -rel;
    if (x_first < 0) x_first = 0;
    long long x_last = E - m < (long long)win.y ? E - m : (long long)win.y;
    if (E - (long long)nb - rel < x_last) x_last = E - (long long)nb - rel;
    for (long long base = x_first; base <= x_last; base += KMP_WAVE) {
        const long long x = base + lane, pos = x + rel;
        const bool ok = match_at(text_a, pa->pat, (uint32_t)m, x, E, win) && pos >= 0 && pos + (long long)nb <= E;
        uint32_t be = 0u, le = 0u;
        if (ok) {
#pragma unroll
            for (uint32_t i = 0; i < 4u; ++i)
                if (i < nb) {
                    const uint32_t c = text[pos + i];
                    be = be << 8 | c;
                    le |= c << (8u * i);
                }
        }
        if (__ballot(ok && compare(little ? le : be, mask, value, want)) != 0ull) return true;
    }
    return false;
}

__global__ void __launch_bounds__(BT_THREADS)
kmp_bytetests_rel_kernel(const unsigned long long *__restrict__ marks, uint64_t stride, uint64_t W, uint64_t n_pkts,
                         const uint4 *__restrict__ tests, const uint32_t *__restrict__ rel_idx, uint32_t n_relative,
                         const kmp_pattern_dev *__restrict__ patterns, const uint8_t *__restrict__ arena, const uint8_t *__restrict__ fold,
                         const uint64_t *__restrict__ pkt_off, const uint32_t *__restrict__ pkt_len, const uint2 *__restrict__ windows,
                         int whole, unsigned long long *__restrict__ rows, unsigned long long *__restrict__ bt_counts,
                         unsigned long long *__restrict__ any)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));       /* the loops below are scalar */
    const uint64_t items = (uint64_t)n_relative * W, step = (uint64_t)gridDim.x * BT_WAVES;
    for (uint64_t item = (uint64_t)blockIdx.x * BT_WAVES + wave; item < items; item += step) {
        const uint64_t r = item / W, j = item - r * W;
        const uint64_t q = rel_idx[r];
        const uint4 a = tests[q * BT_REC];               /* anchor | fold << 31, offset, mask, value */
        const uint32_t nof = tests[q * BT_REC + 1u].x;   /* nbytes | op << 8 | flags << 16 */
        const uint32_t anchor = a.x & 0x7FFFFFFFu;
        unsigned long long cand = marks[(uint64_t)anchor * stride + j];
        if (j == (n_pkts >> 6)) cand &= (1ull << (n_pkts & 63u)) - 1ull;          /* (the marking pass sets no such bit) */
        uint2 win = make_uint2(0u, 0xFFFFFFFFu);
        if (windows && cand) win = windows[anchor];
        const uint32_t want = (BT_OP_BITS >> (3u * ((nof >> 8) & 0xFFu))) & 7u;
        unsigned long long res = 0ull;
        while (cand) {
            const uint32_t bit = (uint32_t)__builtin_ctzll(cand);
            cand &= cand - 1ull;
            const uint64_t k = j * 64u + bit;
            const uint64_t off = pkt_off[k];
            const uint32_t len = pkt_len[k];
            const uint32_t E = whole ? len : text_end(arena + off, len, lane);
            if (bytetest_holds(((a.x >> 31) ? fold : arena) + off, arena + off, patterns + anchor, (int32_t)a.y, nof & 0xFFu,
                               ((nof >> 16) & KMPGPU_BT_LITTLE) != 0u, a.z, a.w, want, E, win, lane))
                res |= 1ull << bit;
        }
        if (lane == 0u) {
            rows[q * stride + j] = res;
            if (res) {
                atomicAdd(bt_counts + q, (unsigned long long)__builtin_popcountll(res));
                atomicOr(any + j, res);
            }
        }
    }
}

}  // namespace

hipError_t kmp_launch_bytetests(bool relative, const unsigned long long *marks, uint64_t stride, uint64_t n_pkts, const uint4 *tests,
                                uint32_t n_bt, const uint32_t *rel_idx, uint32_t n_relative, uint32_t H, const kmp_pattern_dev *patterns,
                                const uint8_t *arena, const uint8_t *fold, const uint64_t *pkt_off, const uint32_t *pkt_len,
                                const void *windows, bool whole, uint32_t max_blocks, unsigned long long *rows,
                                unsigned long long *bt_counts, unsigned long long *any, hipStream_t st)
{
    const uint64_t W = (n_pkts + 63u) / 64u;
    if (n_bt == 0 || W == 0 || n_relative > n_bt) return n_relative > n_bt ? hipErrorInvalidValue : hipSuccess;
    if ((stride & 1u) || W > stride) return hipErrorInvalidValue;
    if (relative) {
        if (n_relative == 0) return hipSuccess;
        const uint64_t items = (uint64_t)n_relative * W;
        uint64_t bx = (items + BT_WAVES - 1u) / BT_WAVES;
        if (bx > max_blocks) bx = max_blocks ? max_blocks : 1u;
        hipLaunchKernelGGL(kmp_bytetests_rel_kernel, dim3((uint32_t)bx), dim3(BT_THREADS), 0, st, marks, stride, W, n_pkts, tests, rel_idx,
                           n_relative, patterns, arena, fold, pkt_off, pkt_len, reinterpret_cast<const uint2 *>(windows), whole ? 1 : 0, rows,
                           bt_counts, any);
        return hipGetLastError();
    }
    if (n_relative == n_bt) return hipSuccess;
    const uint64_t bx = (stride + BT_WAVES - 1u) / BT_WAVES;
    if (bx > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const uint32_t tiles = (n_bt + KMP_BT_TILE - 1u) / KMP_BT_TILE;
    const uint32_t by = (uint32_t)std::min<uint64_t>(std::min(tiles, BT_MAX_BY), std::max<uint64_t>(1u, 1024u / bx));
    const dim3 grid((uint32_t)bx, by);
    if (whole)
        hipLaunchKernelGGL(kmp_bytetests_abs_kernel<true>, grid, dim3(BT_THREADS), 0, st, arena, pkt_off, pkt_len, n_pkts, stride, tests, n_bt, H,
                           reinterpret_cast<ulonglong2 *>(rows), bt_counts, any);
    else
        hipLaunchKernelGGL(kmp_bytetests_abs_kernel<false>, grid, dim3(BT_THREADS), 0, st, arena, pkt_off, pkt_len, n_pkts, stride, tests, n_bt, H,
                           reinterpret_cast<ulonglong2 *>(rows), bt_counts, any);
    return hipGetLastError();
}
