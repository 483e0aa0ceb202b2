/*
 * kmp_chains.hip -- the chain kernel of kmpgpu_scan_chains / kmpgpu_scan_rules on gfx950: 2 .. KMPGPU_CHAIN_MAX contents, each measured
 * from the match of the content before it (kmpgpu_set_chains, kmpgpu.h).  It runs behind the marking pass like the relation kernel
 * (kmp_relations.hip, whose shape this is) and writes one further row of the hit matrix per chain:
 *   rows[c][j]        = for the payloads k of word j: matches (k, s_0, p_0) .. (k, s_{n-1}, p_{n-1}) with
 *                       dmin_i <= s_i - (s_{i-1} + m_{p_{i-1}}) <= dmax_i for every link i = 1 .. n-1
 *   chain_counts[c]   = the set bits of row c
 *   any[j]            = OR over all chains of word j
 *
 * One wavefront takes one (chain, word of 64 payloads), grid-stride.  The candidates are the payloads that hold every content of the
 * chain: the AND of the n pattern rows of that word.  They are decided one after the other from their bytes; the 64 result bits leave
 * with one plain store, one atomic add and one atomic OR.
 *
 * The decision generalises the relation kernel's sweep.  With the bounds of link i clamped to +-(E_k + 99) (no difference of two starts
 * lies outside), lo_i = m_{p_{i-1}} + dlo_i, span_i = dhi_i - dlo_i and the cumulative shifts S_0 = 0, S_i = S_{i-1} + lo_i, write a
 * start of stage i as s_i = x_i + S_i.  Link i then reads 0 <= x_i - x_{i-1} <= span_i: in the shifted coordinate every content lies at
 * or behind the one before it, and at most span_i behind.  So
 *   valid_0(x) = match_0(x)
 *   valid_i(x) = match_i(x + S_i)  and  lastValid_{i-1}(x) >= x - span_i         lastValid_i(x) = the largest x' <= x with valid_i(x')
 * and valid_i(x) holds exactly when some tuple of matches of the first i + 1 contents ends with stage i at x: if any valid x' of stage
 * i - 1 lies in [x - span_i, x], the largest one at or below x does.  The chain holds iff valid_{n-1} holds somewhere.  One ascending
 * sweep over x, a lane per x and 64 per step, decides it: lastValid_{i-1}(x) is the highest set bit at or below the lane in this step's
 * ballot of valid_{i-1}, or stage i - 1's carry from the steps before.  The state is one carry per link.
 * Range: x_0 >= 0, every later x_i >= x_0, and stage i cannot start in front of -S_i, so nothing in front of
 * max(0, max_i(-S_i - (span_1 + .. + span_i))) matters; stage i ends inside the text, x_i <= E_k - m_i - S_i, and the last stage lies at
 * most span_{i+1} + .. + span_{n-1} behind it, so the sweep ends at the smallest of these.  For two contents this is the relation
 * kernel's range.  A stage that no prefix has reached yet (no carry, nothing in this step) ends the step: no later stage can be valid.
 *
 * No run-time register indexing: stage i's constants (S_i, span_i, m, the pattern's bytes, the text it is compared in, its window) and
 * its carry live in lane i of a few VGPRs, loaded by that lane, and are read with v_readlane at the scalar stage index.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kmpgpu.h"
#include "kmp_device.h"
#include "kmp_launch.h"
#include "kmp_sweep_dev.h"

namespace {

constexpr uint32_t CHAIN_THREADS = 256u;
constexpr uint32_t CHAIN_WAVES = CHAIN_THREADS / KMP_WAVE;
constexpr long long NO_CARRY = -(1ll << 40);             /* no valid start so far: below every x - span */

__device__ __forceinline__ uint32_t lane32(uint32_t v, uint32_t l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)l); }

__device__ __forceinline__ long long lane64(long long v, uint32_t l)
{
    const uint32_t lo = lane32((uint32_t)(unsigned long long)v, l), hi = lane32((uint32_t)((unsigned long long)v >> 32), l);
    return (long long)(((unsigned long long)hi << 32) | lo);
}

/* What lane i < n holds of stage i (the lanes behind repeat stage n - 1 and are never read). */
struct Stage {
    long long S, span;           /* cumulative shift, reach of link i (stage 0: 0, unused) */
    long long pat, text;         /* addresses: the pattern's bytes, the payload in the copy of the arena it is compared in */
    uint32_t  m;
    uint2     win;
};

/* The sweep (see the top of the file).  Everything but the lane is wave-uniform, and so is the result.  dmin / dmax: lane i holds the
 * bounds of link i. */
__device__ __forceinline__ bool chain_holds(Stage st, int32_t dmin, int32_t dmax, uint32_t n, uint32_t E32, uint32_t lane)
{
    const long long E = E32, lim = E + KMPGPU_MAX_PATTERN_LEN;
    /* the shifts, stage by stage (scalar), and the range of the sweep */
    long long S = 0, P = 0, x_first = 0, x_last = E - (long long)lane32(st.m, 0);
    st.S = 0; st.span = 0;
    for (uint32_t i = 1; i < n; ++i) {
        const long long lo_b = (int32_t)lane32((uint32_t)dmin, i), hi_b = (int32_t)lane32((uint32_t)dmax, i);
        const long long d_lo = lo_b > -lim ? lo_b : -lim, d_hi = hi_b < lim ? hi_b : lim;
        if (d_lo > d_hi) return false;
        x_last += d_hi - d_lo;                                           /* every stage so far may lie that much further in front */
        S += (long long)lane32(st.m, i - 1u) + d_lo;
        P += d_hi - d_lo;
        if (lane == i) { st.S = S; st.span = d_hi - d_lo; }
        if (-S - P > x_first) x_first = -S - P;
        const long long end_i = E - (long long)lane32(st.m, i) - S;
        if (end_i < x_last) x_last = end_i;
    }
    long long carry = NO_CARRY;                                          /* lane i: the last valid x of stage i in the steps before */
    for (long long base = x_first; base <= x_last; base += KMP_WAVE) {
        const long long x = base + lane;
        uint64_t prev = 0ull;                                            /* this step's ballot of the stage before */
        long long prev_carry = NO_CARRY;
        for (uint32_t i = 0; i < n; ++i) {
            bool ok = true;
            if (i) {
                const uint64_t below = prev & ((2ull << lane) - 1ull);   /* the valid x of stage i - 1 at or below this lane (lane 63: all) */
                const long long last = below ? base + 63 - (long long)__builtin_clzll(below) : prev_carry;
                ok = last >= x - lane64(st.span, i);
            }
            if (__ballot(ok) != 0ull)
                ok = match_at(reinterpret_cast<const uint8_t *>(lane64(st.text, i)), reinterpret_cast<const uint8_t *>(lane64(st.pat, i)),
                              lane32(st.m, i), x + lane64(st.S, i), E, make_uint2(lane32(st.win.x, i), lane32(st.win.y, i))) && ok;
            const uint64_t mb = __ballot(ok);
            if (i + 1u == n) {
                if (mb != 0ull) return true;
                break;
            }
            prev_carry = lane64(carry, i);
            if (mb == 0ull && prev_carry == NO_CARRY) break;            /* no prefix has reached stage i: none reaches a later one */
            prev = mb;
            if (mb != 0ull && lane == i) carry = base + 63 - (long long)__builtin_clzll(mb);
        }
    }
    return false;
}

__global__ void __launch_bounds__(CHAIN_THREADS)
kmp_chains_kernel(const unsigned long long *__restrict__ marks, uint64_t stride, uint64_t W, uint64_t n_pkts,
                  const uint4 *__restrict__ chains, uint32_t n_chains, const kmp_pattern_dev *__restrict__ patterns,
                  const uint8_t *__restrict__ arena, const uint8_t *__restrict__ fold, const uint64_t *__restrict__ pkt_off,
                  const uint32_t *__restrict__ pkt_len, const uint2 *__restrict__ windows, int whole,
                  unsigned long long *__restrict__ rows, unsigned long long *__restrict__ chain_counts,
                  unsigned long long *__restrict__ any)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));       /* the loops below are scalar */
    const uint64_t items = (uint64_t)n_chains * W, step = (uint64_t)gridDim.x * CHAIN_WAVES;
    for (uint64_t item = (uint64_t)blockIdx.x * CHAIN_WAVES + wave; item < items; item += step) {
        const uint64_t c = item / W, j = item - c * W;
        const uint4 *rec = chains + c * KMPGPU_CHAIN_MAX;               /* per link: pattern | fold << 31, dmin, dmax, n */
        const uint32_t n = rec[0].w;
        const uint4 r = rec[lane < n ? lane : n - 1u];                   /* lane i: link i */
        const uint32_t p = r.x & 0x7FFFFFFFu;
        const unsigned long long mine = marks[(uint64_t)p * stride + j];
        unsigned long long cand = ~0ull;
        for (uint32_t i = 0; i < n; ++i) cand &= (unsigned long long)lane64((long long)mine, i);
        if (j == (n_pkts >> 6)) cand &= (1ull << (n_pkts & 63u)) - 1ull;          /* (the marking pass sets no such bit) */
        Stage st;
        st.S = 0; st.span = 0;
        st.pat = (long long)reinterpret_cast<uintptr_t>(patterns[p].pat);
        st.m = 0u;
        st.win = make_uint2(0u, 0xFFFFFFFFu);
        if (cand) {
            st.m = patterns[p].m;
            if (windows) st.win = windows[p];
        }
        unsigned long long res = 0ull;
        while (cand) {
            const uint32_t bit = (uint32_t)__builtin_ctzll(cand);
            cand &= cand - 1ull;
            const uint64_t k = j * 64u + bit;
            const uint64_t off = pkt_off[k];
            const uint32_t len = pkt_len[k];
            const uint32_t E = whole ? len : text_end(arena + off, len, lane);
            st.text = (long long)reinterpret_cast<uintptr_t>(((r.x >> 31) ? fold : arena) + off);
            if (chain_holds(st, (int32_t)r.y, (int32_t)r.z, n, E, lane)) res |= 1ull << bit;
        }
        if (lane == 0u) {
            rows[c * stride + j] = res;
            if (res) {
                atomicAdd(chain_counts + c, (unsigned long long)__builtin_popcountll(res));
                atomicOr(any + j, res);
            }
        }
    }
}

}  // namespace

hipError_t kmp_launch_chains(const unsigned long long *marks, uint64_t stride, uint64_t n_pkts, const uint4 *chains, uint32_t n_chains,
                             const kmp_pattern_dev *patterns, const uint8_t *arena, const uint8_t *fold, const uint64_t *pkt_off,
                             const uint32_t *pkt_len, const void *windows, bool whole, uint32_t max_blocks, unsigned long long *rows,
                             unsigned long long *chain_counts, unsigned long long *any, hipStream_t st)
{
    const uint64_t W = (n_pkts + 63u) / 64u;
    if (n_chains == 0 || W == 0) return hipSuccess;
    if (W > stride) return hipErrorInvalidValue;
    const uint64_t items = (uint64_t)n_chains * W;
    uint64_t bx = (items + CHAIN_WAVES - 1u) / CHAIN_WAVES;
    if (bx > max_blocks) bx = max_blocks ? max_blocks : 1u;
    hipLaunchKernelGGL(kmp_chains_kernel, dim3((uint32_t)bx), dim3(CHAIN_THREADS), 0, st, marks, stride, W, n_pkts, chains, n_chains,
                       patterns, arena, fold, pkt_off, pkt_len, reinterpret_cast<const uint2 *>(windows), whole ? 1 : 0, rows,
                       chain_counts, any);
    return hipGetLastError();
}
