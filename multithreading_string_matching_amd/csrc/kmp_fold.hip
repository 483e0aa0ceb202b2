/*
 * kmp_fold.hip -- the folded copy of an arena for case-insensitive (KMPGPU_PAT_NOCASE) patterns (kmpgpu.h).
 *
 * kmp_fold_kernel writes dst[i] = fold(src[i]) over [0, n16 * 16): ASCII 'A'..'Z' (0x41..0x5A) become 'a'..'z', every
 * other byte is copied as it is.  Folding keeps every offset, every slot's padding and 0x00 against non-0x00, so the
 * packet-start bitmap, the plans and the uniform / packed / pad_clean flags of the original hold for the copy and the
 * scan kernels run on it unchanged ("Case-insensitive patterns").  A pure streaming read-modify-write: every
 * lane moves KMP_FOLD_UNROLL 16-byte vectors, all loads in flight before the first store, non-temporal both ways (each
 * byte is touched once).  One short-lived block per KMP_FOLD_UNROLL * 256 vectors, handed out in order by the hardware.
 *
 * kmp_slot_end_kernel: the end of the furthest slot of an index that is not in arena order (an arena scanned in place,
 * KMPGPU_OPT_REPACK = 0): the fold must not read behind it (kmpgpu.h, "behind the last slot").
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "kmp_launch.h"

namespace {

typedef uint32_t fold_u32x4 __attribute__((ext_vector_type(4)));

constexpr uint32_t KMP_FOLD_THREADS = 256;
constexpr uint32_t KMP_FOLD_UNROLL = 4;

/* SWAR fold of four bytes: t + 0x3F has bit 7 set from 0x41 on, t + 0x25 from 0x5B on (t = x & 0x7F, no carry leaves a
 * byte); their difference in bit 7 marks 0x41..0x5A of the low seven bits, ~x keeps 0xC1..0xDA as they are. */
__device__ __forceinline__ uint32_t fold4(uint32_t x)
{
    const uint32_t t = x & 0x7F7F7F7Fu;
    const uint32_t up = ((t + 0x3F3F3F3Fu) ^ (t + 0x25252525u)) & ~x & 0x80808080u;
    return x | (up >> 2);
}

__global__ void __launch_bounds__(KMP_FOLD_THREADS)
kmp_fold_kernel(const fold_u32x4 *__restrict__ src, fold_u32x4 *__restrict__ dst, uint64_t n16)
{
    const uint64_t base = (uint64_t)blockIdx.x * (KMP_FOLD_THREADS * KMP_FOLD_UNROLL) + threadIdx.x;
    fold_u32x4 v[KMP_FOLD_UNROLL];
    if (base + (KMP_FOLD_UNROLL - 1) * KMP_FOLD_THREADS < n16) {
#pragma unroll
        for (uint32_t k = 0; k < KMP_FOLD_UNROLL; k++) v[k] = __builtin_nontemporal_load(src + base + k * KMP_FOLD_THREADS);
#pragma unroll
        for (uint32_t k = 0; k < KMP_FOLD_UNROLL; k++) {
            fold_u32x4 w = v[k];
            w.x = fold4(w.x); w.y = fold4(w.y); w.z = fold4(w.z); w.w = fold4(w.w);
            __builtin_nontemporal_store(w, dst + base + k * KMP_FOLD_THREADS);
        }
        return;
    }
    /* the last block: every vector checked on its own */
#pragma unroll
    for (uint32_t k = 0; k < KMP_FOLD_UNROLL; k++) {
        const uint64_t i = base + k * KMP_FOLD_THREADS;
        if (i >= n16) break;
        fold_u32x4 w = __builtin_nontemporal_load(src + i);
        w.x = fold4(w.x); w.y = fold4(w.y); w.z = fold4(w.z); w.w = fold4(w.w);
        __builtin_nontemporal_store(w, dst + i);
    }
}

__global__ void __launch_bounds__(KMP_FOLD_THREADS)
kmp_slot_end_kernel(const uint64_t *__restrict__ pkt_off, const uint32_t *__restrict__ pkt_len, uint64_t n, unsigned long long *end)
{
    unsigned long long best = 0;
    for (uint64_t k = (uint64_t)blockIdx.x * KMP_FOLD_THREADS + threadIdx.x; k < n; k += (uint64_t)gridDim.x * KMP_FOLD_THREADS) {
        const uint64_t l16 = ((uint64_t)pkt_len[k] + 15u) & ~15ull;
        const unsigned long long e = pkt_off[k] + (l16 < 16u ? 16u : l16);
        best = e > best ? e : best;
    }
    atomicMax(end, best);
}

}  // namespace

hipError_t kmp_launch_fold(const uint8_t *src, uint8_t *dst, uint64_t bytes, hipStream_t st)
{
    const uint64_t n16 = bytes / 16u;
    if (n16 == 0) return hipSuccess;
    const uint64_t per_block = (uint64_t)KMP_FOLD_THREADS * KMP_FOLD_UNROLL;
    const uint64_t blocks = (n16 + per_block - 1) / per_block;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kmp_fold_kernel, dim3((uint32_t)blocks), dim3(KMP_FOLD_THREADS), 0, st, (const fold_u32x4 *)src, (fold_u32x4 *)dst, n16);
    return hipGetLastError();
}

hipError_t kmp_launch_slot_end(const uint64_t *pkt_off, const uint32_t *pkt_len, uint64_t n, unsigned long long *end, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    const uint64_t blocks = std::min<uint64_t>((n + KMP_FOLD_THREADS - 1) / KMP_FOLD_THREADS, 1024u);
    hipLaunchKernelGGL(kmp_slot_end_kernel, dim3((uint32_t)blocks), dim3(KMP_FOLD_THREADS), 0, st, pkt_off, pkt_len, n, end);
    return hipGetLastError();
}
