/*
 * kmp_links.hip -- kmpgpu_link_rows on gfx950: rows of one context's hit matrix (or rule rows) translated into another context's payload
 * numbering (the definition: kmpgpu.h).  Bit k of an output row is bit map(k) of the source row, for k < n_dst where map(k) exists and is
 * below n_src; every other bit is 0.
 *
 * Shape.  A bitmap map needs the rank of every set bit: kmp_link_rank_kernel leaves per map word the popcount of the words in front of it
 * inside its tile of KMP_LINK_RANK_TILE words and per tile its total, kmp_link_totals_kernel (one block) turns the totals into the tiles'
 * bases and the grand total, which the host compares with n_src before anything is written.  No block waits for another.
 * kmp_link_gather_kernel: a wavefront per output word, a lane per destination payload, grid-stride.  The lane finds its source payload once,
 * then reads its bit of every source row; one ballot forms the output word and lane 0 stores it.  With a bitmap the 64 source payloads of a
 * wavefront are consecutive (at most two words of a row), with an index they lie where the caller put them.  kmp_link_same_kernel, the
 * identity map, is a 16-byte-per-lane copy that clears the bits at n_dst and above.  The rows' popcounts and their OR are not taken here:
 * the copy into the matrix that follows every marking pass is followed by the reduce of kmpgpu_scan_packets where somebody asks for them.
 * Rows x n / 8 bytes each way.  The identity copy runs at the memory's rate; the gather stores 8 bytes per wavefront and row and reaches a
 * fraction of it (DESIGN.md §3.33 has the figures), which a handful of linked rows does not notice: the price of a link is the source's pass.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kmp_launch.h"
#include "kmpgpu.h"

namespace {

constexpr uint32_t RANK_ITEMS = KMP_LINK_RANK_TILE / KMP_BLOCK_THREADS;      /* map words per thread */
static_assert(RANK_ITEMS * KMP_BLOCK_THREADS == KMP_LINK_RANK_TILE, "a tile is a whole number of words per thread");

/* the bits of map word w that stand for payloads below n_dst */
__device__ __forceinline__ unsigned long long map_word(const unsigned long long *__restrict__ map, uint64_t w, uint64_t W, uint64_t n_dst)
{
    if (w >= W) return 0ull;
    const unsigned long long m = map[w];
    const uint32_t tail = (uint32_t)(n_dst & 63u);
    return (w + 1u == W && tail) ? m & ((1ull << tail) - 1ull) : m;
}

/* inclusive sum over the block's KMP_BLOCK_THREADS values; *total: the block's sum.  s_wave: KMP_BLOCK_WAVES words of LDS */
__device__ __forceinline__ unsigned long long block_scan(unsigned long long v, unsigned long long *s_wave, unsigned long long *total)
{
    const uint32_t lane = threadIdx.x & (KMP_WAVE - 1u), wave = threadIdx.x / KMP_WAVE;
    for (uint32_t o = 1u; o < KMP_WAVE; o <<= 1) {
        const unsigned long long up = __shfl_up(v, o);
        if (lane >= o) v += up;
    }
    __syncthreads();                                     /* (the round before has read s_wave) */
    if (lane == KMP_WAVE - 1u) s_wave[wave] = v;
    __syncthreads();
    unsigned long long before = 0ull, all = 0ull;
    for (uint32_t i = 0; i < KMP_BLOCK_WAVES; ++i) {
        if (i < wave) before += s_wave[i];
        all += s_wave[i];
    }
    *total = all;
    return v + before;
}

__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_link_rank_kernel(const unsigned long long *__restrict__ map, uint64_t n_dst, uint64_t W, uint32_t *__restrict__ rank,
                     unsigned long long *__restrict__ tile_total)
{
    __shared__ unsigned long long s_wave[KMP_BLOCK_WAVES];
    const uint64_t w0 = (uint64_t)blockIdx.x * KMP_LINK_RANK_TILE + (uint64_t)threadIdx.x * RANK_ITEMS;
    uint32_t pc[RANK_ITEMS], sum = 0u;
#pragma unroll
    for (uint32_t i = 0; i < RANK_ITEMS; ++i) {
        pc[i] = (uint32_t)__builtin_popcountll(map_word(map, w0 + i, W, n_dst));
        sum += pc[i];
    }
    unsigned long long total;
    uint32_t run = (uint32_t)block_scan(sum, s_wave, &total) - sum;          /* the set bits of the tile in front of this thread's words */
#pragma unroll
    for (uint32_t i = 0; i < RANK_ITEMS; ++i) {
        if (w0 + i < W) rank[w0 + i] = run;
        run += pc[i];
    }
    if (threadIdx.x == 0u) tile_total[blockIdx.x] = total;
}

/* tile_base[i] = the totals of the tiles in front of tile i, in place; tile_base[n_tiles] = the grand total.  One block. */
__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_link_totals_kernel(unsigned long long *__restrict__ tile_base, uint32_t n_tiles)
{
    __shared__ unsigned long long s_wave[KMP_BLOCK_WAVES];
    unsigned long long carry = 0ull;
    for (uint32_t b0 = 0; b0 < n_tiles; b0 += KMP_BLOCK_THREADS) {
        const uint32_t i = b0 + threadIdx.x;
        const unsigned long long v = i < n_tiles ? tile_base[i] : 0ull;
        unsigned long long total;
        const unsigned long long incl = block_scan(v, s_wave, &total);
        if (i < n_tiles) tile_base[i] = carry + incl - v;
        carry += total;
    }
    if (threadIdx.x == 0u) tile_base[n_tiles] = carry;
}

template <int KIND>
__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_link_gather_kernel(const unsigned long long *__restrict__ src_rows, uint64_t src_stride, uint64_t n_src, uint32_t n_rows, uint64_t n_dst,
                       uint64_t W, const unsigned long long *__restrict__ bitmap, const unsigned long long *__restrict__ tile_base,
                       const uint32_t *__restrict__ rank, const uint32_t *__restrict__ index, unsigned long long *__restrict__ dst_rows,
                       uint64_t dst_stride)
{
    const uint32_t lane = threadIdx.x & (KMP_WAVE - 1u);
    const uint64_t wave = (uint64_t)blockIdx.x * KMP_BLOCK_WAVES + threadIdx.x / KMP_WAVE, n_waves = (uint64_t)gridDim.x * KMP_BLOCK_WAVES;
    for (uint64_t j = wave; j < W; j += n_waves) {
        const uint64_t k = j * KMP_WAVE + lane;
        bool has = k < n_dst;
        uint64_t s = 0;
        if (KIND == KMPGPU_LINK_BITMAP) {
            const unsigned long long m = bitmap[j];
            has = has && ((m >> lane) & 1ull) != 0ull;
            s = tile_base[j / KMP_LINK_RANK_TILE] + rank[j] + (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1ull));
        } else {
            if (has) s = index[k];
        }
        has = has && s < n_src;                          /* no load behind the last word of a source row */
        const unsigned long long *p = src_rows + (has ? s >> 6 : 0ull);
        const uint32_t sh = (uint32_t)(s & 63u);
        unsigned long long *out = dst_rows + j;
        for (uint32_t r = 0; r < n_rows; ++r) {
            const bool bit = has && ((p[(uint64_t)r * src_stride] >> sh) & 1ull) != 0ull;
            const unsigned long long word = __ballot(bit);
            if (lane == 0u) out[(uint64_t)r * dst_stride] = word;
        }
    }
}

/* the identity map: pairs of words, the source's and the destination's rows `pairs` apart */
__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_link_same_kernel(const ulonglong2 *__restrict__ src_rows, uint64_t pairs, uint32_t n_rows, uint64_t n_dst, uint64_t W,
                     ulonglong2 *__restrict__ dst_rows)
{
    const uint32_t tail = (uint32_t)(n_dst & 63u);
    const unsigned long long last = tail ? (1ull << tail) - 1ull : ~0ull;
    const uint64_t items = (uint64_t)n_rows * pairs, step = (uint64_t)gridDim.x * KMP_BLOCK_THREADS;
    for (uint64_t i = (uint64_t)blockIdx.x * KMP_BLOCK_THREADS + threadIdx.x; i < items; i += step) {
        const uint64_t w = 2u * (i % pairs);
        ulonglong2 v = src_rows[i];
        v.x = w >= W ? 0ull : w + 1u == W ? v.x & last : v.x;
        v.y = w + 1u >= W ? 0ull : w + 2u == W ? v.y & last : v.y;
        dst_rows[i] = v;
    }
}

}  // namespace

size_t kmp_link_rank_bytes(uint64_t n_dst)
{
    const uint64_t W = (n_dst + 63u) / 64u, tiles = (W + KMP_LINK_RANK_TILE - 1u) / KMP_LINK_RANK_TILE;
    return (size_t)((tiles + 1u) * sizeof(unsigned long long) + W * sizeof(uint32_t));
}

hipError_t kmp_launch_link_rank(const unsigned long long *bitmap, uint64_t n_dst, uint8_t *ws, hipStream_t st)
{
    const uint64_t W = (n_dst + 63u) / 64u, tiles = (W + KMP_LINK_RANK_TILE - 1u) / KMP_LINK_RANK_TILE;
    if (tiles > 0x7FFFFFFFull) return hipErrorInvalidValue;
    unsigned long long *tile_base = reinterpret_cast<unsigned long long *>(ws);
    uint32_t *rank = reinterpret_cast<uint32_t *>(tile_base + tiles + 1u);
    if (tiles) {
        hipLaunchKernelGGL(kmp_link_rank_kernel, dim3((uint32_t)tiles), dim3(KMP_BLOCK_THREADS), 0, st, bitmap, n_dst, W, rank, tile_base);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kmp_link_totals_kernel, dim3(1), dim3(KMP_BLOCK_THREADS), 0, st, tile_base, (uint32_t)tiles);
    return hipGetLastError();
}

hipError_t kmp_launch_link_gather(int kind, const unsigned long long *src_rows, uint64_t src_stride, uint64_t n_src, uint32_t n_rows,
                                  uint64_t n_dst, const void *map, const uint8_t *rank_ws, unsigned long long *dst_rows,
                                  uint64_t dst_stride, hipStream_t st)
{
    const uint64_t W = (n_dst + 63u) / 64u;
    if (n_rows == 0 || W == 0) return hipSuccess;
    if (kind == KMPGPU_LINK_SAME) {
        if (src_stride != dst_stride || (dst_stride & 1u) || n_src != n_dst) return hipErrorInvalidValue;
        const uint64_t pairs = dst_stride / 2u;
        hipLaunchKernelGGL(kmp_link_same_kernel, dim3(kmp_item_blocks((uint64_t)n_rows * pairs)), dim3(KMP_BLOCK_THREADS), 0, st,
                           reinterpret_cast<const ulonglong2 *>(src_rows), pairs, n_rows, n_dst, W, reinterpret_cast<ulonglong2 *>(dst_rows));
        return hipGetLastError();
    }
    const dim3 grid(kmp_group_blocks(n_dst)), block(KMP_BLOCK_THREADS);
    if (kind == KMPGPU_LINK_BITMAP) {
        const uint64_t tiles = (W + KMP_LINK_RANK_TILE - 1u) / KMP_LINK_RANK_TILE;
        const unsigned long long *tile_base = reinterpret_cast<const unsigned long long *>(rank_ws);
        hipLaunchKernelGGL(kmp_link_gather_kernel<KMPGPU_LINK_BITMAP>, grid, block, 0, st, src_rows, src_stride, n_src, n_rows, n_dst, W,
                           static_cast<const unsigned long long *>(map), tile_base, reinterpret_cast<const uint32_t *>(tile_base + tiles + 1u),
                           static_cast<const uint32_t *>(nullptr), dst_rows, dst_stride);
    } else if (kind == KMPGPU_LINK_INDEX) {
        hipLaunchKernelGGL(kmp_link_gather_kernel<KMPGPU_LINK_INDEX>, grid, block, 0, st, src_rows, src_stride, n_src, n_rows, n_dst, W,
                           static_cast<const unsigned long long *>(nullptr), static_cast<const unsigned long long *>(nullptr),
                           static_cast<const uint32_t *>(nullptr), static_cast<const uint32_t *>(map), dst_rows, dst_stride);
    } else {
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
