/*
 * kmp_rules.hip -- the rules kernel of kmpgpu_scan_rules on gfx950: the hit matrix the scan kernels marked (kmp_dev_common.h,
 * mark_match_as; bit k of row i: payload k holds pattern i) is read through the rules' term lists, and gives
 *   rule_rows[r][j]  = AND over the positive terms i of rule r of word j of row i, AND over its negated terms of the complement,
 *                      with the bits of index n_pkts and above cleared
 *   rule_counts[r]   = the set bits of rule row r   (payloads that rule r matches)
 *   any[j]           = OR over all rule rows of word j
 *
 * Shape, as the reduce of kmp_marks.hip: lanes cover column words, two per lane (one 16-byte load per term, one 16-byte store per
 * rule); a group of cl = 1..64 lanes (of one wavefront) covers 2 cl words of a rule's row, the 256 / cl groups of a block take
 * different rules.  So tens of thousands of rules over a few words keep every lane busy, and a few rules over millions of words
 * stream in full 1 KiB wavefront loads.  A rule's 16-byte head carries its first two terms (two row loads in flight per lane: rules
 * of one or two terms need nothing else), the further terms come four at a time (one 16-byte load of the term list, then four row
 * loads in flight); lists are filled up with repeats of a term of the rule, so no load hangs on a condition.  A lane whose
 * accumulator has run empty reads no further quad of the rule.  A rule's popcount is
 * summed over its group's lanes and added with one atomic per (block, rule); the column OR is gathered in LDS and ORed into
 * any[] with one atomic per (block, word).
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kmpgpu.h"
#include "kmp_launch.h"

namespace {

constexpr uint32_t RULES_THREADS = 256u;
constexpr uint32_t RULES_MAX_BY = 1024u;     /* blocks in y: further rules are taken in further rounds of the grid */

/* the two words of term `term`'s row in this lane's columns, complemented for a negated term */
__device__ __forceinline__ ulonglong2 term_words(const ulonglong2 *__restrict__ marks, uint64_t pairs, uint64_t pair, uint32_t term)
{
    ulonglong2 v = marks[(uint64_t)(term & ~KMPGPU_RULE_NOT) * pairs + pair];
    const unsigned long long flip = (term & KMPGPU_RULE_NOT) ? ~0ull : 0ull;
    v.x ^= flip; v.y ^= flip;
    return v;
}

__global__ void __launch_bounds__(RULES_THREADS)
kmp_rules_kernel(const ulonglong2 *__restrict__ marks, uint64_t pairs, uint64_t n_pkts, const uint4 *__restrict__ heads,
                 const uint4 *__restrict__ quads, uint32_t n_rules, uint32_t clog, ulonglong2 *__restrict__ rule_rows,
                 unsigned long long *__restrict__ rule_counts, unsigned long long *__restrict__ any)
{
    __shared__ unsigned long long s_any[128];

    const uint32_t cl = 1u << clog;
    const uint32_t t = threadIdx.x;
    const uint32_t sub = t & (cl - 1u);                  /* lane inside its group */
    const uint32_t grp = t >> clog;
    const uint32_t groups = RULES_THREADS >> clog;
    const uint64_t pair = (uint64_t)blockIdx.x * cl + sub;       /* column words 2 pair, 2 pair + 1 */
    const bool col_ok = pair < pairs;

    /* the payloads behind these two words: all 64, the first n_pkts % 64 in the last word, none in the padding word of an odd W */
    const uint64_t full = n_pkts >> 6;
    const unsigned long long last = (1ull << (n_pkts & 63u)) - 1ull;
    const unsigned long long mx = 2u * pair < full ? ~0ull : 2u * pair == full ? last : 0ull;
    const unsigned long long my = 2u * pair + 1u < full ? ~0ull : 2u * pair + 1u == full ? last : 0ull;

    if (t < 2u * cl) s_any[t] = 0ull;

    unsigned long long ax = 0ull, ay = 0ull;
    for (uint64_t rb = (uint64_t)blockIdx.y * groups; rb < n_rules; rb += (uint64_t)gridDim.y * groups) {
        const uint64_t r = rb + grp;
        ulonglong2 acc = make_ulonglong2(0ull, 0ull);
        if (col_ok && r < n_rules) {
            const uint4 h = heads[r];                    /* x, y: the quads [x, y) hold the terms behind the first two, z, w: the first two terms */
            {
                const ulonglong2 v0 = term_words(marks, pairs, pair, h.z);
                const ulonglong2 v1 = term_words(marks, pairs, pair, h.w);
                acc.x = mx & v0.x & v1.x;
                acc.y = my & v0.y & v1.y;
            }
            for (uint32_t q = h.x; q < h.y && (acc.x | acc.y) != 0ull; ++q) {
                const uint4 tq = quads[q];
                const ulonglong2 v0 = term_words(marks, pairs, pair, tq.x);
                const ulonglong2 v1 = term_words(marks, pairs, pair, tq.y);
                const ulonglong2 v2 = term_words(marks, pairs, pair, tq.z);
                const ulonglong2 v3 = term_words(marks, pairs, pair, tq.w);
                acc.x &= (v0.x & v1.x) & (v2.x & v3.x);
                acc.y &= (v0.y & v1.y) & (v2.y & v3.y);
            }
            rule_rows[r * pairs + pair] = acc;
        }
        ax |= acc.x; ay |= acc.y;
        uint32_t pc = (uint32_t)__builtin_popcountll(acc.x) + (uint32_t)__builtin_popcountll(acc.y);
        for (uint32_t o = cl >> 1; o > 0u; o >>= 1) pc += (uint32_t)__shfl_xor((int)pc, (int)o);    /* inside the group */
        if (sub == 0u && pc != 0u && r < n_rules) atomicAdd(rule_counts + r, (unsigned long long)pc);
    }
    __syncthreads();
    if (ax) atomicOr(&s_any[2u * sub], ax);
    if (ay) atomicOr(&s_any[2u * sub + 1u], ay);
    __syncthreads();
    if (t < 2u * cl) {
        const unsigned long long w = s_any[t];
        const uint64_t col = 2ull * blockIdx.x * cl + t;
        if (w && col < 2ull * pairs) atomicOr(any + col, w);
    }
}

}  // namespace

hipError_t kmp_launch_rules(const unsigned long long *marks, uint64_t stride, uint64_t n_pkts, const uint4 *heads, const uint4 *quads,
                            uint32_t n_rules, unsigned long long *rule_rows, unsigned long long *rule_counts, unsigned long long *any,
                            hipStream_t st)
{
    if (n_rules == 0 || stride == 0) return hipSuccess;
    if ((stride & 1u) || n_pkts > stride * 64u) return hipErrorInvalidValue;
    const uint64_t pairs = stride / 2u;
    uint32_t clog = 0;
    while ((1ull << clog) < pairs && clog < 6u) ++clog;
    const uint32_t cl = 1u << clog;
    const uint64_t bx = (pairs + cl - 1u) / cl;
    if (bx > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const uint64_t groups = RULES_THREADS >> clog;
    uint64_t by = (n_rules + groups - 1u) / groups;
    by = by < RULES_MAX_BY ? by : RULES_MAX_BY;
    hipLaunchKernelGGL(kmp_rules_kernel, dim3((uint32_t)bx, (uint32_t)by), dim3(RULES_THREADS), 0, st,
                       reinterpret_cast<const ulonglong2 *>(marks), pairs, n_pkts, heads, quads, n_rules, clog,
                       reinterpret_cast<ulonglong2 *>(rule_rows), rule_counts, any);
    return hipGetLastError();
}
