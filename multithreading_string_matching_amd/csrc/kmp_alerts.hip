/*
 * kmp_alerts.hip -- kmpgpu_scan_alerts: the set bits of a row family of the hit matrix as (payload, row) records, sorted by payload,
 * then row, built on the device (kmpgpu.h).  gfx950.
 *
 * The matrix is row-major (row i, word j holds payloads 64 j .. 64 j + 63), the list is payload-major: a transposing compaction.
 *
 *   kmp_alerts_count_kernel   cnt[k] = set bits of column k, written as the "length" 16 cnt[k] (0xFFFFFFFF where cnt[k] == 0: "rejected")
 *   kmp_scan_local_kernel, kmp_scan_totals_kernel   of kmp_prep.hip, through kmp_launch_compact_scan: the byte offset of every payload's
 *                             first 16-byte record, totals = {16 x records, payloads with a record}
 *   kmp_alerts_fill_kernel    the same walk; every payload's records at its offset, ascending rows
 *
 * The walk.  A wavefront owns KMP_ALERTS_WORDS = 4 adjacent column words (256 payloads) and takes the rows 64 at a time: lane i loads the
 * 32 bytes of row r0 + i (two 16-byte loads; rows are 16-byte aligned and of an even number of words), so the four wavefronts of a block
 * read one whole 128-byte line of every row.  A column word whose any[] word is 0 is never transposed, four such words in a row are not
 * read at all; a 64 x 64 block of bits that is all zero (one __any) is skipped too.  Otherwise the block is transposed in registers
 * with six butterfly steps of __shfl_xor: lane p then holds the mask of the rows r0 .. r0 + 63 that hit payload 64 j + p.  The count adds
 * its popcount; the fill writes one record per set bit in ctz order -- ascending rows -- at the payload's running position, one 16-byte
 * store each.  No atomic decides a position: the order is that of the scan, the same for every run.
 * Chosen over one ballot per set bit of the step's OR: the transpose costs the same 12 cross-lane moves per non-empty block whatever its
 * density, a ballot per column costs up to 64 of them, and the cheap case of both -- an empty block -- is the same __any.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "kmp_device.h"
#include "kmp_launch.h"

namespace {

typedef uint32_t alert_u32x4 __attribute__((ext_vector_type(4)));

constexpr uint32_t KMP_ALERTS_WORDS = 4;          /* column words a wavefront owns: 32 bytes of every row */
constexpr uint32_t KMP_ALERTS_BLOCKS = 1024;      /* grid cap of both kernels: rounds past 1024 x 4 x 4 x 64 = 1 048 576 payloads */

__device__ __forceinline__ uint64_t shfl_xor64(uint64_t v, uint32_t s)
{
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, (int)s), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), (int)s);
    return ((uint64_t)hi << 32) | lo;
}

/* Lane i holds row i of a 64 x 64 bit matrix (bit p: column p); returns its column `lane` (bit i: row i).  Six steps: the matrix in 2 x 2
 * blocks of s x s bits, the two off-diagonal ones swapped between lane and lane ^ s. */
__device__ __forceinline__ uint64_t transpose64(uint64_t x, uint32_t lane)
{
#pragma unroll
    for (uint32_t s = 32u; s; s >>= 1) {
        const uint64_t m = ~0ull / ((1ull << s) + 1ull);          /* the bits whose index has bit s clear */
        const uint64_t y = shfl_xor64(x, s);
        x = (lane & s) ? ((x & ~m) | ((y & ~m) >> s)) : ((x & m) | ((y & m) << s));
    }
    return x;
}

template <bool FILL>
__device__ __forceinline__ void alerts_walk(const unsigned long long *__restrict__ rows, uint64_t stride, uint32_t n_rows, uint64_t n_pkts,
                                            const unsigned long long *__restrict__ any, const uint64_t *__restrict__ loc_off,
                                            const uint64_t *__restrict__ blk_bytes, uint32_t *__restrict__ cnt_len,
                                            alert_u32x4 *__restrict__ recs, uint64_t max_records)
{
    const uint32_t lane = threadIdx.x & (KMP_WAVE - 1u), wid = threadIdx.x >> 6;
    const uint64_t W = (n_pkts + 63u) / 64u;
    const uint64_t n_quads = (W + KMP_ALERTS_WORDS - 1u) / KMP_ALERTS_WORDS;
    for (uint64_t q = (uint64_t)blockIdx.x * KMP_BLOCK_WAVES + wid; q < n_quads; q += (uint64_t)gridDim.x * KMP_BLOCK_WAVES) {
        const uint64_t j0 = q * KMP_ALERTS_WORDS;
        unsigned long long a[KMP_ALERTS_WORDS];
        uint32_t cnt[KMP_ALERTS_WORDS];
        uint64_t pos[KMP_ALERTS_WORDS];
        unsigned long long live = 0ull;
#pragma unroll
        for (uint32_t u = 0; u < KMP_ALERTS_WORDS; ++u) {
            a[u] = (j0 + u < W) ? any[j0 + u] : 0ull;
            live |= a[u];
            cnt[u] = 0u;
            pos[u] = 0ull;
            const uint64_t k = (j0 + u) * 64u + lane;
            if (FILL && a[u] && k < n_pkts) pos[u] = (blk_bytes[k / KMP_SCAN_TILE] + loc_off[k]) / 16u;
        }
        if (live) {
            for (uint32_t r0 = 0; r0 < n_rows; r0 += KMP_WAVE) {
                const uint32_t r = r0 + lane;
                ulonglong2 v0 = make_ulonglong2(0ull, 0ull), v1 = v0;
                if (r < n_rows) {
                    /* (j0 + 1 < stride always: stride is even and j0 < W <= stride) */
                    const unsigned long long *p = rows + (uint64_t)r * stride + j0;
                    v0 = *reinterpret_cast<const ulonglong2 *>(p);
                    if (j0 + 2u < stride) v1 = *reinterpret_cast<const ulonglong2 *>(p + 2);
                }
                const unsigned long long w[KMP_ALERTS_WORDS] = {v0.x, v0.y, v1.x, v1.y};
#pragma unroll
                for (uint32_t u = 0; u < KMP_ALERTS_WORDS; ++u) {
                    if (!a[u] || !__any(w[u] != 0ull)) continue;                 /* (both the same for every lane) */
                    const uint64_t k = (j0 + u) * 64u + lane;
                    uint64_t t = transpose64(w[u], lane);
                    if (k >= n_pkts) t = 0ull;                                   /* bits at n_pkts and above never give a record */
                    if (!FILL) cnt[u] += (uint32_t)__builtin_popcountll(t);
                    else
                        while (t) {
                            const uint32_t b = (uint32_t)__builtin_ctzll(t);
                            t &= t - 1ull;
                            if (pos[u] < max_records) {
                                alert_u32x4 rec;
                                rec.x = (uint32_t)k; rec.y = (uint32_t)(k >> 32); rec.z = r0 + b; rec.w = 0u;
                                recs[pos[u]] = rec;
                            }
                            ++pos[u];
                        }
                }
            }
        }
        if (!FILL) {
#pragma unroll
            for (uint32_t u = 0; u < KMP_ALERTS_WORDS; ++u) {
                const uint64_t k = (j0 + u) * 64u + lane;
                if (k < n_pkts) cnt_len[k] = cnt[u] ? 16u * cnt[u] : 0xFFFFFFFFu;
            }
        }
    }
}

__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_alerts_count_kernel(const unsigned long long *__restrict__ rows, uint64_t stride, uint32_t n_rows, uint64_t n_pkts,
                        const unsigned long long *__restrict__ any, uint32_t *__restrict__ cnt_len)
{
    alerts_walk<false>(rows, stride, n_rows, n_pkts, any, nullptr, nullptr, cnt_len, nullptr, 0ull);
}

__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_alerts_fill_kernel(const unsigned long long *__restrict__ rows, uint64_t stride, uint32_t n_rows, uint64_t n_pkts,
                       const unsigned long long *__restrict__ any, const uint64_t *__restrict__ loc_off,
                       const uint64_t *__restrict__ blk_bytes, alert_u32x4 *__restrict__ recs, uint64_t max_records)
{
    alerts_walk<true>(rows, stride, n_rows, n_pkts, any, loc_off, blk_bytes, nullptr, recs, max_records);
}

uint32_t alerts_blocks(uint64_t n_pkts)
{
    const uint64_t per_block = (uint64_t)KMP_BLOCK_WAVES * KMP_ALERTS_WORDS * 64u;
    return (uint32_t)std::min<uint64_t>((n_pkts + per_block - 1) / per_block, KMP_ALERTS_BLOCKS);
}

}  // namespace

hipError_t kmp_launch_alerts_count(const unsigned long long *rows, uint64_t stride, uint32_t n_rows, uint64_t n_pkts,
                                   const unsigned long long *any, uint8_t *ws, hipStream_t st)
{
    if (n_pkts == 0) return hipSuccess;
    if ((stride & 1u) || stride * 64u < n_pkts || (uint64_t)n_rows * 16u > 0xFFFFFFFEull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kmp_alerts_count_kernel, dim3(alerts_blocks(n_pkts)), dim3(KMP_BLOCK_THREADS), 0, st, rows, stride, n_rows, n_pkts, any,
                       kmp_compact_ws(ws, n_pkts).len);
    return hipGetLastError();
}

hipError_t kmp_launch_alerts_fill(const unsigned long long *rows, uint64_t stride, uint32_t n_rows, uint64_t n_pkts,
                                  const unsigned long long *any, uint8_t *ws, void *recs, uint64_t max_records, hipStream_t st)
{
    if (n_pkts == 0 || max_records == 0) return hipSuccess;
    if ((stride & 1u) || stride * 64u < n_pkts) return hipErrorInvalidValue;
    const kmp_compact_view w = kmp_compact_ws(ws, n_pkts);
    hipLaunchKernelGGL(kmp_alerts_fill_kernel, dim3(alerts_blocks(n_pkts)), dim3(KMP_BLOCK_THREADS), 0, st, rows, stride, n_rows, n_pkts, any,
                       w.loc_off, w.blk_bytes, reinterpret_cast<alert_u32x4 *>(recs), max_records);
    return hipGetLastError();
}
