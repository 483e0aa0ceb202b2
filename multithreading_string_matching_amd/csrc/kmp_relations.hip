/*
 * kmp_relations.hip -- the relation kernel of kmpgpu_scan_relations / kmpgpu_scan_rules on gfx950: distance / within between two
 * patterns (kmpgpu_set_relations, kmpgpu.h).  It runs behind the marking pass, reads the hit matrix that pass filled (bit k of
 * row i: payload k holds an in-window match of pattern i) and writes one further row per relation:
 *   rows[q][j]        = for the payloads k of word j: some match (k, sa, a) and some match (k, sb, b) with
 *                       dmin <= sb - (sa + m_a) <= dmax
 *   rel_counts[q]     = the set bits of row q
 *   any[j]            = OR over all relations of word j
 *
 * Where the work comes from: a payload can only satisfy relation q when it holds both patterns, so the candidates of (q, j) are
 * marks[a][j] & marks[b][j] -- on real traffic a handful of payloads per relation.  One wavefront takes one (q, j), grid-stride, and
 * decides its candidates one after the other from the payloads' bytes; it then writes the 64 result bits with one plain store
 * (nobody else writes that word), adds their number to rel_counts[q] and ORs them into any[j] with one atomic each.
 *
 * The decision is exact and uses no memory that grows with the payload: a single ascending sweep, one lane per offset x, 64 offsets
 * per step.  With lo = m_a + dmin and span = dmax - dmin (the bounds clamped to +-(E_k + 99) first: no difference of two starts lies
 * outside, so the unbounded sides disappear), a start sb = x + lo of b pairs with exactly the starts sa in [x - span, x] of a.  Lane x
 * computes matchA(x) and matchB(x + lo); lastA(x), the largest start of a at or below x, is the highest set bit at or below the lane
 * in the step's ballot of matchA, or the carry from the steps before; the pair exists iff some lane has matchB(x + lo) and
 * lastA(x) >= x - span.  The sweep covers x in [max(0, -lo - span), min(E_k - m_b - lo, E_k - m_a + span)]: no start of a lies in
 * front of 0, none that matters in front of -lo - span, and behind the upper end either b has left the text or the last a is out of
 * reach.
 * A match is what the marking pass marks: s + m <= E_k (E_k = the payload's first 0x00 unless the pass runs whole payloads: found by
 * the wavefront in 16-byte loads before the sweep), first <= s <= last where windows are set, and the bytes of a pattern of the
 * nocase set compared in the folded copy of the arena against the folded pattern (kmp_pattern_dev.pat holds it folded).  A lane
 * compares its own offset byte by byte and leaves at the first difference; the loop ends when no lane is left.  No byte at or behind
 * E_k is compared, and the 16-byte loads stay inside round_up(L_k, 16), i.e. inside the payload's slot.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kmpgpu.h"
#include "kmp_device.h"
#include "kmp_launch.h"
#include "kmp_sweep_dev.h"                /* text_end, match_at: shared with kmp_chains.hip */

namespace {

constexpr uint32_t REL_THREADS = 256u;
constexpr uint32_t REL_WAVES = REL_THREADS / KMP_WAVE;

/* The sweep (see the top of the file).  Everything but the lane is wave-uniform, and so is the result. */
__device__ __forceinline__ bool relation_holds(const uint8_t *__restrict__ text_a, const uint8_t *__restrict__ text_b,
                                               const kmp_pattern_dev *__restrict__ pa, const kmp_pattern_dev *__restrict__ pb,
                                               int32_t dmin, int32_t dmax, uint32_t E32, uint2 win_a, uint2 win_b, uint32_t lane)
{
    const long long E = E32, m_a = pa->m, m_b = pb->m, lim = E + KMPGPU_MAX_PATTERN_LEN;
    const long long d_lo = (long long)dmin > -lim ? (long long)dmin : -lim;
    const long long d_hi = (long long)dmax < lim ? (long long)dmax : lim;
    if (d_lo > d_hi) return false;
    const long long lo = m_a + d_lo, span = d_hi - d_lo;
    const long long x_first = -lo - span > 0 ? -lo - span : 0;
    const long long end_b = E - m_b - lo, end_a = E - m_a + span;
    const long long x_last = end_b < end_a ? end_b : end_a;
    long long carry = -(1ll << 40);                      /* no start of a so far: below every x - span */
    for (long long base = x_first; base <= x_last; base += KMP_WAVE) {
        const long long x = base + lane;
        const bool a = match_at(text_a, pa->pat, (uint32_t)m_a, x, E, win_a);
        const bool b = match_at(text_b, pb->pat, (uint32_t)m_b, x + lo, E, win_b);
        const uint64_t ma = __ballot(a);
        const uint64_t below = ma & ((2ull << lane) - 1ull);               /* the starts of a at or below this lane (lane 63: all) */
        const long long last = below ? base + 63 - (long long)__builtin_clzll(below) : carry;
        if (__ballot(b && last >= x - span) != 0ull) return true;
        if (ma) carry = base + 63 - (long long)__builtin_clzll(ma);
    }
    return false;
}

__global__ void __launch_bounds__(REL_THREADS)
kmp_relations_kernel(const unsigned long long *__restrict__ marks, uint64_t stride, uint64_t W, uint64_t n_pkts,
                     const uint4 *__restrict__ relations, uint32_t n_rel, const kmp_pattern_dev *__restrict__ patterns,
                     const uint8_t *__restrict__ arena, const uint8_t *__restrict__ fold, const uint64_t *__restrict__ pkt_off,
                     const uint32_t *__restrict__ pkt_len, const uint2 *__restrict__ windows, int whole,
                     unsigned long long *__restrict__ rows, unsigned long long *__restrict__ rel_counts,
                     unsigned long long *__restrict__ any)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));       /* the loops below are scalar */
    const uint64_t items = (uint64_t)n_rel * W, step = (uint64_t)gridDim.x * REL_WAVES;
    for (uint64_t item = (uint64_t)blockIdx.x * REL_WAVES + wave; item < items; item += step) {
        const uint64_t q = item / W, j = item - q * W;
        const uint4 r = relations[q];                    /* a | fold << 31, b | fold << 31, dmin, dmax */
        const uint32_t a = r.x & 0x7FFFFFFFu, b = r.y & 0x7FFFFFFFu;
        unsigned long long cand = marks[(uint64_t)a * stride + j] & marks[(uint64_t)b * stride + j];
        if (j == (n_pkts >> 6)) cand &= (1ull << (n_pkts & 63u)) - 1ull;          /* (the marking pass sets no such bit) */
        uint2 win_a = make_uint2(0u, 0xFFFFFFFFu), win_b = win_a;
        if (windows && cand) { win_a = windows[a]; win_b = windows[b]; }
        unsigned long long res = 0ull;
        while (cand) {
            const uint32_t bit = (uint32_t)__builtin_ctzll(cand);
            cand &= cand - 1ull;
            const uint64_t k = j * 64u + bit;
            const uint64_t off = pkt_off[k];
            const uint32_t len = pkt_len[k];
            const uint32_t E = whole ? len : text_end(arena + off, len, lane);
            if (relation_holds(((r.x >> 31) ? fold : arena) + off, ((r.y >> 31) ? fold : arena) + off, patterns + a, patterns + b,
                               (int32_t)r.z, (int32_t)r.w, E, win_a, win_b, lane))
                res |= 1ull << bit;
        }
        if (lane == 0u) {
            rows[q * stride + j] = res;
            if (res) {
                atomicAdd(rel_counts + q, (unsigned long long)__builtin_popcountll(res));
                atomicOr(any + j, res);
            }
        }
    }
}

}  // namespace

hipError_t kmp_launch_relations(const unsigned long long *marks, uint64_t stride, uint64_t n_pkts, const uint4 *relations, uint32_t n_rel,
                                const kmp_pattern_dev *patterns, const uint8_t *arena, const uint8_t *fold, const uint64_t *pkt_off,
                                const uint32_t *pkt_len, const void *windows, bool whole, uint32_t max_blocks, unsigned long long *rows,
                                unsigned long long *rel_counts, unsigned long long *any, hipStream_t st)
{
    const uint64_t W = (n_pkts + 63u) / 64u;
    if (n_rel == 0 || W == 0) return hipSuccess;
    if (W > stride) return hipErrorInvalidValue;
    const uint64_t items = (uint64_t)n_rel * W;
    uint64_t bx = (items + REL_WAVES - 1u) / REL_WAVES;
    if (bx > max_blocks) bx = max_blocks ? max_blocks : 1u;
    hipLaunchKernelGGL(kmp_relations_kernel, dim3((uint32_t)bx), dim3(REL_THREADS), 0, st, marks, stride, W, n_pkts, relations, n_rel,
                       patterns, arena, fold, pkt_off, pkt_len, reinterpret_cast<const uint2 *>(windows), whole ? 1 : 0, rows,
                       rel_counts, any);
    return hipGetLastError();
}
