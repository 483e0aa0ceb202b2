/*
 * kmp_marks.hip -- the reduce of kmpgpu_scan_packets on gfx950: the hit matrix the scan kernels marked (kmp_dev_common.h,
 * mark_match_as; bit k of row i: payload k holds pattern i) is read once, and gives
 *   pkt_counts[i] = the set bits of row i        (payloads that hold pattern i)
 *   any[j]        = OR over all rows of word j   (payloads that hold some pattern)
 *
 * Shape: lanes cover column words, two per lane (one 16-byte load); a group of cl = 1..64 lanes (of one wavefront) covers
 * 2 cl words of a row, the 256 / cl groups of a block take different rows.  So a matrix of a few words per row and tens of
 * thousands of rows (70 000 patterns over a hundred payloads) keeps every lane busy and spreads over many blocks, and a
 * matrix of a few rows and millions of words streams in full 1 KiB wavefront loads.  A row's popcount is summed over its
 * group's lanes and added with one atomic per (block, row); the column OR is gathered in LDS and ORed into any[] with one
 * atomic per (block, word).
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kmp_launch.h"

namespace {

constexpr uint32_t MARKS_THREADS = 256u;
constexpr uint32_t MARKS_RPT = 8u;           /* rows per lane per round: eight 16-byte loads in flight */

__global__ void __launch_bounds__(MARKS_THREADS)
kmp_marks_reduce_kernel(const ulonglong2 *__restrict__ marks, uint32_t n_rows, uint64_t pairs, uint32_t clog,
                        unsigned long long *__restrict__ pkt_counts, unsigned long long *__restrict__ any)
{
    __shared__ unsigned long long s_any[128];

    const uint32_t cl = 1u << clog;
    const uint32_t t = threadIdx.x;
    const uint32_t sub = t & (cl - 1u);                  /* lane inside its group */
    const uint32_t grp = t >> clog;
    const uint32_t groups = MARKS_THREADS >> clog;
    const uint64_t pair = (uint64_t)blockIdx.x * cl + sub;       /* column words 2 pair, 2 pair + 1 */
    const bool col_ok = pair < pairs;
    const uint64_t rows_per_round = (uint64_t)groups * MARKS_RPT;

    if (t < 2u * cl) s_any[t] = 0ull;

    unsigned long long ax = 0ull, ay = 0ull;
    for (uint64_t rb = (uint64_t)blockIdx.y * rows_per_round; rb < n_rows; rb += (uint64_t)gridDim.y * rows_per_round) {
        ulonglong2 v[MARKS_RPT];
#pragma unroll
        for (uint32_t i = 0; i < MARKS_RPT; ++i) {
            const uint64_t r = rb + grp + (uint64_t)i * groups;
            v[i] = make_ulonglong2(0ull, 0ull);
            if (col_ok && r < n_rows) v[i] = marks[r * pairs + pair];
        }
#pragma unroll
        for (uint32_t i = 0; i < MARKS_RPT; ++i) {
            const uint64_t r = rb + grp + (uint64_t)i * groups;
            ax |= v[i].x; ay |= v[i].y;
            uint32_t pc = (uint32_t)__builtin_popcountll(v[i].x) + (uint32_t)__builtin_popcountll(v[i].y);
            for (uint32_t o = cl >> 1; o > 0u; o >>= 1) pc += (uint32_t)__shfl_xor((int)pc, (int)o);    /* inside the group */
            if (sub == 0u && pc != 0u && r < n_rows) atomicAdd(pkt_counts + r, (unsigned long long)pc);
        }
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

hipError_t kmp_launch_marks_reduce(const unsigned long long *marks, uint32_t n_rows, uint64_t stride, unsigned long long *pkt_counts,
                                   unsigned long long *any, hipStream_t st)
{
    if (n_rows == 0 || stride == 0) return hipSuccess;
    if (stride & 1u) return hipErrorInvalidValue;
    const uint64_t pairs = stride / 2u;
    uint32_t clog = 0;
    while ((1ull << clog) < pairs && clog < 6u) ++clog;
    const uint32_t cl = 1u << clog;
    const uint64_t bx = (pairs + cl - 1u) / cl;
    if (bx > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const uint64_t rows_per_round = (uint64_t)(MARKS_THREADS >> clog) * MARKS_RPT;
    /* a few rounds of rows per block when there are many rows; the y dimension stays below its limit */
    uint64_t by = (n_rows + rows_per_round - 1u) / rows_per_round;
    by = by < 65535u ? by : 65535u;
    hipLaunchKernelGGL(kmp_marks_reduce_kernel, dim3((uint32_t)bx, (uint32_t)by), dim3(MARKS_THREADS), 0, st,
                       reinterpret_cast<const ulonglong2 *>(marks), n_rows, pairs, clog, pkt_counts, any);
    return hipGetLastError();
}
