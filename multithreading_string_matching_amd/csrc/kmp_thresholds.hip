/*
 * kmp_thresholds.hip -- kmpgpu_scan_thresholds: how often a rule has hit per tracker inside a sliding time window (kmpgpu.h).  gfx950.
 *
 * n[q][k] counts the base hits j <= k of payload k's tracker with T[k] - T[j] < window, T the running maximum of the caller's timestamps.
 * In an order that groups the payloads by tracker and keeps capture order inside a tracker (a stable sort), those j are a contiguous
 * stretch [lo, i] of sorted positions that ends at k's own position i: T does not decrease along a tracker's run, so "same tracker and
 * young enough" is false up to lo and true from lo on.  With C the inclusive prefix sum of the base bits in sorted order,
 * n = C[i] - C[lo - 1].
 *
 *   kmp_thr_reduce_kernel<MaxU64>, kmp_thr_scan_kernel<MaxU64, *>   T = the inclusive max-scan of ts, in place, 64-bit
 *   kmp_thr_keys_kernel         the source or destination address of every payload, the key of the address sort
 *   (kmp_launch_flowbits_order  the stable rocPRIM sort, the inverse order and the head flags: kmp_flowbits.hip, for the flows its own cache)
 *   kmp_thr_tsort_kernel        Tsorted[i] = T[order[i]], once per track and call, so the search reads one array
 *   per threshold:
 *   kmp_thr_gather_kernel       C[i] = base[r][order[i]], four sorted positions a thread, 16-byte loads and stores
 *   kmp_thr_reduce_kernel<SumU32>, kmp_thr_scan_kernel<SumU32, *>   C = its inclusive prefix sum, in place
 *   kmp_thr_pass_kernel         a lane per payload, in payload order: i = inv[k], a binary search for lo over [0, i] on (key, Tsorted),
 *                               n, the comparison, and one ballot for the word of the pass row
 *   kmp_thr_final_kernel        alert[r] = base[r] & the pass rows of r's thresholds, word-wise; counts and any[]
 *
 * The search is over (key, Tsorted) and not inside a precomputed run start: the predicate is monotone over all of [0, i], so no third
 * array, no scan that makes it and nothing to cache per track; the price is a second load (the key) per step, which is issued together with
 * the first and so adds no latency to the chain of dependent steps.  KMPGPU_THR_BY_RULE has no keys and no order: the identity.
 *
 * No block waits on another: a tile scan is reduce, the aggregates' scan (the same kernels, recursively), the tiles from their carry-in,
 * as kmp_flowbits.hip's.  A wavefront scans its 64 partial results with cross-lane moves; LDS holds a block's four wavefront totals alone.
 * No atomic decides a value: the final pass adds popcounts and ORs words.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "kmpgpu.h"
#include "kmp_device.h"
#include "kmp_launch.h"

namespace {

constexpr uint32_t THR_FINAL_MAX_BY = 1024u;     /* blocks in y of the final pass: further rules in further rounds */

static_assert(KMP_SCAN_ITEMS == 4u, "a thread's four items are one or two 16-byte loads");

/* the two scans: the running maximum of 64-bit times, the prefix sum of 32-bit hit counts */
struct MaxU64 {
    typedef unsigned long long V;
    static __device__ __forceinline__ V id() { return 0ull; }
    static __device__ __forceinline__ V op(V a, V b) { return a > b ? a : b; }
    static __device__ __forceinline__ V up(V v, uint32_t o) { return (V)__shfl_up((long long)v, o); }
    static __device__ __forceinline__ void load(const V *p, V out[4])
    {
        const ulonglong2 a = *reinterpret_cast<const ulonglong2 *>(p), b = *reinterpret_cast<const ulonglong2 *>(p + 2);
        out[0] = a.x; out[1] = a.y; out[2] = b.x; out[3] = b.y;
    }
    static __device__ __forceinline__ void store(V *p, const V in[4])
    {
        *reinterpret_cast<ulonglong2 *>(p) = make_ulonglong2(in[0], in[1]);
        *reinterpret_cast<ulonglong2 *>(p + 2) = make_ulonglong2(in[2], in[3]);
    }
};
struct SumU32 {
    typedef uint32_t V;
    static __device__ __forceinline__ V id() { return 0u; }
    static __device__ __forceinline__ V op(V a, V b) { return a + b; }
    static __device__ __forceinline__ V up(V v, uint32_t o) { return (V)__shfl_up((int)v, o); }
    static __device__ __forceinline__ void load(const V *p, V out[4])
    {
        const uint4 a = *reinterpret_cast<const uint4 *>(p);
        out[0] = a.x; out[1] = a.y; out[2] = a.z; out[3] = a.w;
    }
    static __device__ __forceinline__ void store(V *p, const V in[4]) { *reinterpret_cast<uint4 *>(p) = make_uint4(in[0], in[1], in[2], in[3]); }
};

/* inclusive scan over the wavefront's lanes, in lane order */
template <class O>
__device__ __forceinline__ typename O::V thr_wave_scan(typename O::V v, uint32_t lane)
{
#pragma unroll
    for (uint32_t o = 1u; o < KMP_WAVE; o <<= 1) {
        const typename O::V p = O::up(v, o);
        if (lane >= o) v = O::op(p, v);
    }
    return v;
}

/* The four items of the thread whose first is `base`, combined in order into loc[0..3] (inclusive); identities at n and behind.  The
 * array holds a multiple of four items, so the 16-byte loads of a thread with an item below n stay inside it. */
template <class O>
__device__ __forceinline__ void thr_load_items(const typename O::V *__restrict__ data, uint64_t n, uint64_t base, typename O::V loc[KMP_SCAN_ITEMS])
{
    typename O::V raw[KMP_SCAN_ITEMS] = {O::id(), O::id(), O::id(), O::id()};
    if (base < n) O::load(data + base, raw);
    loc[0] = base < n ? raw[0] : O::id();
#pragma unroll
    for (uint32_t j = 1; j < KMP_SCAN_ITEMS; ++j) loc[j] = O::op(loc[j - 1u], base + j < n ? raw[j] : O::id());
}

template <class O>
__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_thr_reduce_kernel(const typename O::V *__restrict__ data, uint64_t n, typename O::V *__restrict__ agg)
{
    typedef typename O::V V;
    __shared__ V s_w[KMP_BLOCK_WAVES];
    const uint32_t lane = threadIdx.x & (KMP_WAVE - 1u), wid = threadIdx.x >> 6;
    V loc[KMP_SCAN_ITEMS];
    thr_load_items<O>(data, n, (uint64_t)blockIdx.x * KMP_SCAN_TILE + (uint64_t)threadIdx.x * KMP_SCAN_ITEMS, loc);
    const V v = thr_wave_scan<O>(loc[KMP_SCAN_ITEMS - 1u], lane);
    if (lane == KMP_WAVE - 1u) s_w[wid] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        V t = s_w[0];
#pragma unroll
        for (uint32_t x = 1; x < KMP_BLOCK_WAVES; ++x) t = O::op(t, s_w[x]);
        agg[blockIdx.x] = t;
    }
}

/* In place.  INCLUSIVE: data[i] = data[0] o .. o data[i], carry[tile] in front where carry is given (the payloads' level);
 * else data[i] = data[0] o .. o data[i - 1] (the aggregates: what comes out are the carry-ins of the level below). */
template <class O, bool INCLUSIVE>
__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_thr_scan_kernel(typename O::V *__restrict__ data, const typename O::V *__restrict__ carry, uint64_t n)
{
    typedef typename O::V V;
    __shared__ V s_w[KMP_BLOCK_WAVES];
    const uint32_t lane = threadIdx.x & (KMP_WAVE - 1u), wid = threadIdx.x >> 6;
    const uint64_t base = (uint64_t)blockIdx.x * KMP_SCAN_TILE + (uint64_t)threadIdx.x * KMP_SCAN_ITEMS;
    V loc[KMP_SCAN_ITEMS];
    thr_load_items<O>(data, n, base, loc);
    const V v = thr_wave_scan<O>(loc[KMP_SCAN_ITEMS - 1u], lane);
    if (lane == KMP_WAVE - 1u) s_w[wid] = v;
    /* what lies in front of this thread inside its wavefront */
    V ex = O::up(v, 1u);
    if (lane == 0u) ex = O::id();
    __syncthreads();
    V front = carry ? carry[blockIdx.x] : O::id();
    for (uint32_t x = 0; x < wid; ++x) front = O::op(front, s_w[x]);
    ex = O::op(front, ex);
    if (base >= n) return;
    /* the results at n and behind (inside the array's last four) are never read */
    V out[KMP_SCAN_ITEMS];
    if (INCLUSIVE) {
#pragma unroll
        for (uint32_t j = 0; j < KMP_SCAN_ITEMS; ++j) out[j] = O::op(ex, loc[j]);
    } else {
        out[0] = ex;
#pragma unroll
        for (uint32_t j = 1; j < KMP_SCAN_ITEMS; ++j) out[j] = O::op(ex, loc[j - 1u]);
    }
    O::store(data + base, out);
}

__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_thr_keys_kernel(const uint4 *__restrict__ meta, uint64_t n, uint32_t dst, uint32_t *__restrict__ keys)
{
    const uint64_t k = (uint64_t)blockIdx.x * KMP_BLOCK_THREADS + threadIdx.x;
    if (k >= n) return;
    const uint4 m = meta[k];                         /* kmpgpu_pkt_meta: src_ip, dst_ip first */
    keys[k] = dst ? m.y : m.x;
}

__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_thr_tsort_kernel(const unsigned long long *__restrict__ T, const uint32_t *__restrict__ order, uint64_t n,
                     unsigned long long *__restrict__ Ts)
{
    const uint64_t i = (uint64_t)blockIdx.x * KMP_BLOCK_THREADS + threadIdx.x;
    if (i < n) Ts[i] = T[order[i]];
}

/* order == NULL: the identity.  C holds a multiple of four items, and so does what lies behind order[n] in its buffer (inv[]). */
__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_thr_gather_kernel(const unsigned long long *__restrict__ row, uint64_t n, const uint32_t *__restrict__ order, uint32_t *__restrict__ C)
{
    const uint64_t base = ((uint64_t)blockIdx.x * KMP_BLOCK_THREADS + threadIdx.x) * KMP_SCAN_ITEMS;
    if (base >= n) return;
    uint32_t k[KMP_SCAN_ITEMS], c[KMP_SCAN_ITEMS];
    if (order) SumU32::load(order + base, k);
    else {
#pragma unroll
        for (uint32_t j = 0; j < KMP_SCAN_ITEMS; ++j) k[j] = (uint32_t)(base + j);
    }
#pragma unroll
    for (uint32_t j = 0; j < KMP_SCAN_ITEMS; ++j) c[j] = base + j < n ? (uint32_t)((row[k[j] >> 6] >> (k[j] & 63u)) & 1ull) : 0u;
    SumU32::store(C + base, c);
}

/* KEYED: inv, keys are the track's order; else the identity and one tracker.  Ts == NULL: no window, every earlier payload of the tracker
 * counts.  wc == NULL: a payload without a base hit needs no count (its alert bit is 0 whatever the pass bit is). */
template <bool KEYED>
__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_thr_pass_kernel(const unsigned long long *__restrict__ row, uint64_t n, const uint32_t *__restrict__ inv, const uint32_t *__restrict__ keys,
                    const unsigned long long *__restrict__ Ts, const uint32_t *__restrict__ C, uint32_t type, uint32_t count,
                    unsigned long long window, unsigned long long *__restrict__ pass_row, uint32_t *__restrict__ wc)
{
    const uint32_t lane = threadIdx.x & (KMP_WAVE - 1u);
    /* the wavefront's 64 payloads are bit 0..63 of column word w */
    const uint64_t w = (uint64_t)blockIdx.x * KMP_BLOCK_WAVES + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t k = w * KMP_WAVE + lane;
    if (w * KMP_WAVE >= n) return;                   /* (the whole wavefront; its word, if the row has it, stays 0) */
    bool pass = false;
    if (k < n && (wc || ((row[w] >> lane) & 1ull))) {
        const uint32_t i = KEYED ? inv[k] : (uint32_t)k;
        const uint32_t key = KEYED ? keys[i] : 0u;
        const unsigned long long t = Ts ? Ts[i] : 0ull;
        /* the first position of [0, i] that is k's tracker and inside the window; i itself is */
        uint32_t lo = 0u, hi = i;
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            bool in = true;
            if (KEYED) in = keys[mid] == key;
            if (Ts) in = in && (t - Ts[mid] < window);      /* (the difference is looked at for k's tracker alone, where it is >= 0) */
            if (in) hi = mid; else lo = mid + 1u;
        }
        const uint32_t cnt = C[i] - (lo ? C[lo - 1u] : 0u);
        if (wc) wc[k] = cnt;
        pass = type == KMPGPU_THR_AT_LEAST ? cnt >= count : type == KMPGPU_THR_AT_MOST ? cnt <= count : cnt == count;
    }
    const unsigned long long word = __ballot(pass);
    if (lane == 0u) pass_row[w] = word;
}

/* of_rule[r] = {first, number} of rule r's thresholds in qlist[], which names their pass rows.  A lane per column word, blocks in y over
 * the rules. */
__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_thr_final_kernel(const unsigned long long *__restrict__ rule_rows, const unsigned long long *__restrict__ pass_rows, uint64_t stride,
                     const uint2 *__restrict__ of_rule, const uint32_t *__restrict__ qlist, uint32_t n_rules,
                     unsigned long long *__restrict__ alert_rows, unsigned long long *__restrict__ counts, unsigned long long *__restrict__ any)
{
    const uint32_t lane = threadIdx.x & (KMP_WAVE - 1u);
    const uint64_t j = (uint64_t)blockIdx.x * KMP_BLOCK_THREADS + threadIdx.x;
    const bool ok = j < stride;
    unsigned long long seen = 0ull;
    for (uint32_t r = blockIdx.y; r < n_rules; r += gridDim.y) {
        const uint2 t = of_rule[r];
        unsigned long long acc = 0ull;
        if (ok) {
            acc = rule_rows[(uint64_t)r * stride + j];
            for (uint32_t x = 0; x < t.y && acc; ++x) acc &= pass_rows[(uint64_t)qlist[t.x + x] * stride + j];
            alert_rows[(uint64_t)r * stride + j] = acc;
        }
        seen |= acc;
        uint32_t pc = (uint32_t)__builtin_popcountll(acc);
#pragma unroll
        for (uint32_t o = KMP_WAVE >> 1; o > 0u; o >>= 1) pc += (uint32_t)__shfl_xor((int)pc, (int)o);
        if (lane == 0u && pc != 0u) atomicAdd(counts + r, (unsigned long long)pc);
    }
    if (ok && seen) atomicOr(any + j, seen);
}

/* items a scan over n rounds its array up to: whole 16-byte loads */
uint64_t thr_pad(uint64_t n) { return (n + 3u) & ~3ull; }

uint32_t thr_blocks(uint64_t n) { return (uint32_t)((n + KMP_BLOCK_THREADS - 1u) / KMP_BLOCK_THREADS); }

/* The inclusive (top) or exclusive scan of data[n] in place: one block where it is one tile, else reduce, the aggregates' exclusive scan in
 * `agg` (and behind it theirs), the tiles from their carry-in. */
template <class O>
hipError_t thr_scan(typename O::V *data, uint64_t n, typename O::V *agg, bool top, uint32_t *launches, hipStream_t st)
{
    const uint64_t tiles = (n + KMP_SCAN_TILE - 1u) / KMP_SCAN_TILE;
    if (tiles > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const typename O::V *carry = nullptr;
    if (tiles > 1u) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(kmp_thr_reduce_kernel<O>), dim3((uint32_t)tiles), dim3(KMP_BLOCK_THREADS), 0, st, data, n, agg);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        ++*launches;
        e = thr_scan<O>(agg, tiles, agg + thr_pad(tiles), false, launches, st);
        if (e != hipSuccess) return e;
        carry = agg;
    }
    if (top) hipLaunchKernelGGL(HIP_KERNEL_NAME(kmp_thr_scan_kernel<O, true>), dim3((uint32_t)tiles), dim3(KMP_BLOCK_THREADS), 0, st, data, carry, n);
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(kmp_thr_scan_kernel<O, false>), dim3((uint32_t)tiles), dim3(KMP_BLOCK_THREADS), 0, st, data, carry, n);
    ++*launches;
    return hipGetLastError();
}

}  // namespace

uint64_t kmp_thresholds_pad(uint64_t n) { return thr_pad(n); }

size_t kmp_thresholds_agg_bytes(uint64_t n)
{
    uint64_t items = 0;
    for (uint64_t t = n; t > KMP_SCAN_TILE;) { t = (t + KMP_SCAN_TILE - 1u) / KMP_SCAN_TILE; items += thr_pad(t); }
    return (size_t)(items * sizeof(unsigned long long));
}

hipError_t kmp_launch_thresholds_time(unsigned long long *T, uint64_t n, uint8_t *agg, uint32_t *launches, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    return thr_scan<MaxU64>(T, n, reinterpret_cast<unsigned long long *>(agg), true, launches, st);
}

hipError_t kmp_launch_thresholds_keys(const uint4 *meta, uint64_t n, bool dst, uint32_t *keys, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    if (n > 0xFFFFFFFEull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kmp_thr_keys_kernel, dim3(thr_blocks(n)), dim3(KMP_BLOCK_THREADS), 0, st, meta, n, dst ? 1u : 0u, keys);
    return hipGetLastError();
}

hipError_t kmp_launch_thresholds_tsort(const unsigned long long *T, const uint8_t *order_buf, uint64_t n, unsigned long long *Ts, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    const kmp_order_view o = kmp_flowbits_order_view(order_buf, n);
    hipLaunchKernelGGL(kmp_thr_tsort_kernel, dim3(thr_blocks(n)), dim3(KMP_BLOCK_THREADS), 0, st, T, o.order, n, Ts);
    return hipGetLastError();
}

hipError_t kmp_launch_thresholds_count(const unsigned long long *rule_row, uint64_t n, const uint8_t *order_buf, uint32_t *C, uint8_t *agg,
                                       uint32_t *launches, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    if (n > 0xFFFFFFFEull) return hipErrorInvalidValue;
    const uint32_t *order = order_buf ? kmp_flowbits_order_view(order_buf, n).order : nullptr;
    hipLaunchKernelGGL(kmp_thr_gather_kernel, dim3(thr_blocks((n + KMP_SCAN_ITEMS - 1u) / KMP_SCAN_ITEMS)), dim3(KMP_BLOCK_THREADS), 0, st, rule_row,
                       n, order, C);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    ++*launches;
    return thr_scan<SumU32>(C, n, reinterpret_cast<uint32_t *>(agg), true, launches, st);
}

hipError_t kmp_launch_thresholds_pass(const unsigned long long *rule_row, uint64_t n, const uint8_t *order_buf, const unsigned long long *Ts,
                                      const uint32_t *C, uint32_t type, uint32_t count, unsigned long long window,
                                      unsigned long long *pass_row, uint32_t *window_counts, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    if (n > 0xFFFFFFFEull) return hipErrorInvalidValue;
    if (window == KMPGPU_THR_NO_WINDOW) Ts = nullptr;
    else if (!Ts) return hipErrorInvalidValue;
    if (order_buf) {
        const kmp_order_view o = kmp_flowbits_order_view(order_buf, n);
        hipLaunchKernelGGL(kmp_thr_pass_kernel<true>, dim3(thr_blocks(n)), dim3(KMP_BLOCK_THREADS), 0, st, rule_row, n, o.inv, o.keys, Ts, C, type,
                           count, window, pass_row, window_counts);
    } else
        hipLaunchKernelGGL(kmp_thr_pass_kernel<false>, dim3(thr_blocks(n)), dim3(KMP_BLOCK_THREADS), 0, st, rule_row, n, (const uint32_t *)nullptr,
                           (const uint32_t *)nullptr, Ts, C, type, count, window, pass_row, window_counts);
    return hipGetLastError();
}

hipError_t kmp_launch_thresholds_final(const unsigned long long *rule_rows, const unsigned long long *pass_rows, uint64_t stride,
                                       const uint32_t *table, uint32_t n_rules, unsigned long long *alert_rows, unsigned long long *counts,
                                       unsigned long long *any, hipStream_t st)
{
    if (n_rules == 0 || stride == 0) return hipSuccess;
    const uint64_t bx = (stride + KMP_BLOCK_THREADS - 1u) / KMP_BLOCK_THREADS;
    if (bx > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kmp_thr_final_kernel, dim3((uint32_t)bx, std::min(n_rules, THR_FINAL_MAX_BY)), dim3(KMP_BLOCK_THREADS), 0, st, rule_rows,
                       pass_rows, stride, reinterpret_cast<const uint2 *>(table), table + 2u * (size_t)n_rules, n_rules, alert_rows, counts, any);
    return hipGetLastError();
}
