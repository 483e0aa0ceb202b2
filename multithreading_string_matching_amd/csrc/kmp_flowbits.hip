/*
 * kmp_flowbits.hip -- kmpgpu_scan_flowbits: the flow bits of kmpgpu_set_flowbits carried along every flow's payloads (kmpgpu.h).  gfx950.
 *
 * For one bit a payload's effect is a function {0,1} -> {0,1}; 32 of them are an element (f0, f1) of two masks: bit X of f0 is what the
 * payload makes of X = 0, of f1 of X = 1.  `f then g` is h0 = (f0 & g1) | (~f0 & g0), h1 = (f1 & g1) | (~f1 & g0): associative, not
 * commutative, identity (0, ~0).  The state before a payload is the composition of its flow's earlier payloads applied to 0: an exclusive
 * scan in flow order that restarts at every flow's first payload.
 *
 *   rocprim::radix_sort_pairs  (flow_of[k], k) sorted by the flow id's significant bits, stably: a flow's payloads stay in capture order.
 *                              The values come from a counting iterator; no atomic decides an order
 *   kmp_fb_heads_kernel        inv[order[i]] = i and head[i] = the key changes at sorted position i; head[n] = 1
 *   per level of the bit graph (kmp_rowtables.h, kmp_pack_flowbits):
 *   kmp_fb_build_kernel        a lane per payload, in payload order: the base rows of the level's acting rules are one word per wavefront
 *                              (its 64 payloads; each lane takes its own bit), the lower levels' bits come from the payload's own word of
 *                              before32[].  The rules are evaluated once for x = 0 and once for x = 1, and the element goes to the
 *                              payload's sorted position.  THE RESTART IS IN THE ELEMENT: a flow's first payload stores the constant
 *                              function (F(0), F(0)), which forgets whatever is composed in front of it -- so the scan below is a plain
 *                              one and no aggregate carries a flag
 *   kmp_fb_reduce_kernel       one aggregate per tile of KMP_SCAN_TILE elements       } only above one tile; the aggregates are
 *   kmp_fb_scan_kernel<false>  the aggregates' exclusive scan in place: the carry-ins } scanned by the same three kernels, recursively
 *   kmp_fb_scan_kernel<true>   every tile from its carry-in: before32[order[i]] |= the exclusive result applied to 0 (0 at a head), and
 *                              flow_state[flow] |= the inclusive result at a flow's last payload
 *   kmp_fb_rows_kernel         a lane per payload, one ballot per bit of the level: the bit's before row, 64 payloads a word
 *   kmp_fb_final_kernel        alert[r] = base[r] & the tests' before rows (or their complements), word-wise; counts and any[]
 *
 * No block waits on another: the tile scan is reduce, scan of the aggregates, scan from the carry-in, as kmp_prep.hip's.  A wavefront scans
 * its 64 partial results with cross-lane moves (no LDS); LDS holds the four wavefront totals of a block alone.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include "kmpgpu.h"
#include "kmp_device.h"
#include "kmp_launch.h"

namespace {

constexpr uint32_t FB_FINAL_MAX_BY = 1024u;      /* blocks in y of the final pass: further rules in further rounds */

/* f, then g */
__device__ __forceinline__ uint2 fb_then(uint2 f, uint2 g)
{
    return make_uint2((f.x & g.y) | (~f.x & g.x), (f.y & g.y) | (~f.y & g.x));
}

/* inclusive scan over the wavefront's lanes, in lane order */
__device__ __forceinline__ uint2 fb_wave_scan(uint2 v, uint32_t lane)
{
#pragma unroll
    for (uint32_t o = 1u; o < KMP_WAVE; o <<= 1) {
        const uint2 p = make_uint2((uint32_t)__shfl_up((int)v.x, o), (uint32_t)__shfl_up((int)v.y, o));
        if (lane >= o) v = fb_then(p, v);
    }
    return v;
}

/* The order buffer: order[n], inv[n], the sorted keys[n] (32 bits each), head[n + 1] (bytes), rocPRIM's temporary storage. */
struct FbOrder {
    uint32_t *order, *inv, *keys;
    uint8_t  *head;
    void     *tmp;
    size_t    used;
};
size_t fb_order_used(uint64_t n) { return (size_t)((13u * n + 1u + 255u) & ~255ull); }
FbOrder fb_order(uint8_t *buf, uint64_t n)
{
    FbOrder o;
    o.order = reinterpret_cast<uint32_t *>(buf);
    o.inv = o.order + n;
    o.keys = o.inv + n;
    o.head = reinterpret_cast<uint8_t *>(o.keys + n);
    o.used = fb_order_used(n);
    o.tmp = buf + o.used;
    return o;
}

/* the flow id's bits that can differ */
uint32_t fb_key_bits(uint64_t n_flows)
{
    uint32_t b = 1u;
    while (b < 32u && ((n_flows - 1u) >> b) != 0u) ++b;
    return b;
}

hipError_t fb_sort_run(void *tmp, size_t &tmp_bytes, const uint32_t *flow_of, const FbOrder &o, uint64_t n, uint64_t n_flows, hipStream_t st)
{
    return rocprim::radix_sort_pairs(tmp, tmp_bytes, flow_of, o.keys, rocprim::counting_iterator<uint32_t>(0u), o.order, (size_t)n, 0u,
                                     fb_key_bits(n_flows), st);
}

__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_fb_heads_kernel(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ order, uint64_t n, uint32_t *__restrict__ inv,
                    uint8_t *__restrict__ head)
{
    const uint64_t i = (uint64_t)blockIdx.x * KMP_BLOCK_THREADS + threadIdx.x;
    if (i < n) {
        head[i] = (i == 0 || keys[i - 1] != keys[i]) ? 1u : 0u;
        inv[order[i]] = (uint32_t)i;
    }
    if (i == n) head[n] = 1u;                        /* (the grid covers n + 1 positions) */
}

/* acting[2 a], acting[2 a + 1]: {rule, lower bits tested set, lower bits tested clear, self}, {a0, a1, 0, 0} (kmp_rowtables.h) */
__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_fb_build_kernel(const unsigned long long *__restrict__ rule_rows, uint64_t stride, uint64_t n, const uint4 *__restrict__ acting,
                    uint32_t n_act, const uint32_t *__restrict__ before32, const uint32_t *__restrict__ inv, const uint8_t *__restrict__ head,
                    uint2 *__restrict__ elems)
{
    const uint32_t lane = threadIdx.x & (KMP_WAVE - 1u);
    /* the wavefront's 64 payloads are bit 0..63 of column word w of every row */
    const uint64_t w = (uint64_t)blockIdx.x * KMP_BLOCK_WAVES + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t k = w * KMP_WAVE + lane;
    if (w * KMP_WAVE >= n) return;                   /* (the whole wavefront) */
    const uint32_t B = k < n ? before32[k] : 0u;
    uint32_t v0 = 0u, v1 = ~0u;
    for (uint32_t a = 0; a < n_act; ++a) {
        const uint4 t = acting[2u * a], f = acting[2u * a + 1u];
        const unsigned long long base = rule_rows[(uint64_t)t.x * stride + w];
        const bool c = ((base >> lane) & 1ull) != 0ull && (B & t.y) == t.y && (B & t.z) == 0u;
        /* the tests see the state BEFORE the payload -- x itself for the rule's own bit --, the actions the running value */
        if (c && !(t.w & 1u)) v0 = (v0 & f.y) | (~v0 & f.x);
        if (c && !(t.w & 2u)) v1 = (v1 & f.y) | (~v1 & f.x);
    }
    if (k < n) {
        const uint32_t i = inv[k];
        elems[i] = make_uint2(v0, head[i] ? v0 : v1);
    }
}

/* The four elements of thread t of tile `tile`, composed in order into loc[0..3] (inclusive); identities at n and behind.  elems holds a
 * multiple of four elements, so the two 16-byte loads of a thread with an element below n stay inside it. */
__device__ __forceinline__ void fb_load_items(const uint2 *__restrict__ elems, uint64_t n, uint64_t base, uint2 loc[KMP_SCAN_ITEMS])
{
    static_assert(KMP_SCAN_ITEMS == 4u, "two 16-byte loads per thread");
    uint4 a = make_uint4(0u, ~0u, 0u, ~0u), b = a;
    if (base < n) {
        a = *reinterpret_cast<const uint4 *>(elems + base);
        b = *reinterpret_cast<const uint4 *>(elems + base + 2u);
    }
    const uint2 id = make_uint2(0u, ~0u);
    loc[0] = base < n ? make_uint2(a.x, a.y) : id;
    loc[1] = fb_then(loc[0], base + 1u < n ? make_uint2(a.z, a.w) : id);
    loc[2] = fb_then(loc[1], base + 2u < n ? make_uint2(b.x, b.y) : id);
    loc[3] = fb_then(loc[2], base + 3u < n ? make_uint2(b.z, b.w) : id);
}

__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_fb_reduce_kernel(const uint2 *__restrict__ elems, uint64_t n, uint2 *__restrict__ agg)
{
    __shared__ uint2 s_w[KMP_BLOCK_WAVES];
    const uint32_t lane = threadIdx.x & (KMP_WAVE - 1u), wid = threadIdx.x >> 6;
    uint2 loc[KMP_SCAN_ITEMS];
    fb_load_items(elems, n, (uint64_t)blockIdx.x * KMP_SCAN_TILE + (uint64_t)threadIdx.x * KMP_SCAN_ITEMS, loc);
    const uint2 v = fb_wave_scan(loc[KMP_SCAN_ITEMS - 1u], lane);
    if (lane == KMP_WAVE - 1u) s_w[wid] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint2 t = s_w[0];
#pragma unroll
        for (uint32_t x = 1; x < KMP_BLOCK_WAVES; ++x) t = fb_then(t, s_w[x]);
        agg[blockIdx.x] = t;
    }
}

/* TOP = false: elems[i] = the composition of elems[0 .. i), in place (carry[tile] in front where carry is given).
 * TOP = true: elems are the payloads' in sorted order; the results go to before32 and flow_state and elems stay. */
template <bool TOP>
__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_fb_scan_kernel(uint2 *__restrict__ elems, const uint2 *__restrict__ carry, uint64_t n, const uint32_t *__restrict__ order,
                   const uint8_t *__restrict__ head, const uint32_t *__restrict__ flow_of, uint32_t *__restrict__ before32,
                   uint32_t *__restrict__ flow_state)
{
    __shared__ uint2 s_w[KMP_BLOCK_WAVES];
    const uint32_t lane = threadIdx.x & (KMP_WAVE - 1u), wid = threadIdx.x >> 6;
    const uint64_t base = (uint64_t)blockIdx.x * KMP_SCAN_TILE + (uint64_t)threadIdx.x * KMP_SCAN_ITEMS;
    uint2 loc[KMP_SCAN_ITEMS];
    fb_load_items(elems, n, base, loc);
    const uint2 v = fb_wave_scan(loc[KMP_SCAN_ITEMS - 1u], lane);
    if (lane == KMP_WAVE - 1u) s_w[wid] = v;
    /* what lies in front of this thread inside its wavefront */
    uint2 ex = make_uint2((uint32_t)__shfl_up((int)v.x, 1u), (uint32_t)__shfl_up((int)v.y, 1u));
    if (lane == 0u) ex = make_uint2(0u, ~0u);
    __syncthreads();
    uint2 front = carry ? carry[blockIdx.x] : make_uint2(0u, ~0u);
    for (uint32_t x = 0; x < wid; ++x) front = fb_then(front, s_w[x]);
    ex = fb_then(front, ex);
    if (base >= n) return;
    if (!TOP) {
        /* the exclusive results of the four; those at n and behind are never read */
        const uint2 e1 = fb_then(ex, loc[0]), e2 = fb_then(ex, loc[1]), e3 = fb_then(ex, loc[2]);
        *reinterpret_cast<uint4 *>(elems + base) = make_uint4(ex.x, ex.y, e1.x, e1.y);
        *reinterpret_cast<uint4 *>(elems + base + 2u) = make_uint4(e2.x, e2.y, e3.x, e3.y);
        return;
    }
#pragma unroll
    for (uint32_t j = 0; j < KMP_SCAN_ITEMS; ++j) {
        const uint64_t i = base + j;
        if (i >= n) break;
        const uint2 before = j ? fb_then(ex, loc[j - 1u]) : ex, after = fb_then(ex, loc[j]);
        const uint32_t k = order[i];
        /* applied to 0: the f0 mask.  Bits of other levels are the identity here and add nothing */
        if (!head[i] && before.x) before32[k] |= before.x;
        if (head[i + 1u] && after.x) flow_state[flow_of[k]] |= after.x;
    }
}

__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_fb_rows_kernel(const uint32_t *__restrict__ before32, uint64_t n, uint32_t mask, uint64_t stride, unsigned long long *__restrict__ rows)
{
    const uint32_t lane = threadIdx.x & (KMP_WAVE - 1u);
    const uint64_t w = (uint64_t)blockIdx.x * KMP_BLOCK_WAVES + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t k = w * KMP_WAVE + lane;
    if (w * KMP_WAVE >= n) return;                   /* (the whole wavefront; its word, if the row has it, stays 0) */
    const uint32_t B = k < n ? before32[k] : 0u;
    for (uint32_t m = mask; m; m &= m - 1u) {
        const uint32_t b = (uint32_t)__builtin_ctz(m);
        const unsigned long long word = __ballot((B >> b) & 1u);
        if (lane == 0u) rows[(uint64_t)b * stride + w] = word;
    }
}

/* tests[r] = {bits tested set, bits tested clear, NOALERT, 0}.  A lane per column word, blocks in y over the rules. */
__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_fb_final_kernel(const unsigned long long *__restrict__ rule_rows, const unsigned long long *__restrict__ before_rows, uint64_t stride,
                    const uint4 *__restrict__ tests, uint32_t n_rules, unsigned long long *__restrict__ alert_rows,
                    unsigned long long *__restrict__ counts, unsigned long long *__restrict__ any)
{
    const uint32_t lane = threadIdx.x & (KMP_WAVE - 1u);
    const uint64_t j = (uint64_t)blockIdx.x * KMP_BLOCK_THREADS + threadIdx.x;
    const bool ok = j < stride;
    unsigned long long seen = 0ull;
    for (uint32_t r = blockIdx.y; r < n_rules; r += gridDim.y) {
        const uint4 t = tests[r];
        unsigned long long acc = 0ull;
        if (ok) {
            acc = t.z ? 0ull : rule_rows[(uint64_t)r * stride + j];
            for (uint32_t m = t.x; m && acc; m &= m - 1u) acc &= before_rows[(uint64_t)__builtin_ctz(m) * stride + j];
            for (uint32_t m = t.y; m && acc; m &= m - 1u) acc &= ~before_rows[(uint64_t)__builtin_ctz(m) * stride + j];
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

/* elements a scan over n rounds its buffer up to: whole 16-byte pairs of loads */
uint64_t fb_pad(uint64_t n) { return (n + 3u) & ~3ull; }

uint32_t fb_payload_blocks(uint64_t n) { return (uint32_t)((n + KMP_BLOCK_THREADS - 1u) / KMP_BLOCK_THREADS); }

/* The scan of elems[n]: one block where it is one tile, else reduce, the aggregates' scan in `agg` (and behind it theirs), the tiles. */
hipError_t fb_scan(uint2 *elems, uint64_t n, uint2 *agg, bool top, const uint32_t *order, const uint8_t *head, const uint32_t *flow_of,
                   uint32_t *before32, uint32_t *flow_state, uint32_t *launches, hipStream_t st)
{
    const uint64_t tiles = (n + KMP_SCAN_TILE - 1u) / KMP_SCAN_TILE;
    if (tiles > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const uint2 *carry = nullptr;
    if (tiles > 1u) {
        hipLaunchKernelGGL(kmp_fb_reduce_kernel, dim3((uint32_t)tiles), dim3(KMP_BLOCK_THREADS), 0, st, elems, n, agg);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        ++*launches;
        e = fb_scan(agg, tiles, agg + fb_pad(tiles), false, nullptr, nullptr, nullptr, nullptr, nullptr, launches, st);
        if (e != hipSuccess) return e;
        carry = agg;
    }
    if (top)
        hipLaunchKernelGGL(kmp_fb_scan_kernel<true>, dim3((uint32_t)tiles), dim3(KMP_BLOCK_THREADS), 0, st, elems, carry, n, order, head, flow_of,
                           before32, flow_state);
    else
        hipLaunchKernelGGL(kmp_fb_scan_kernel<false>, dim3((uint32_t)tiles), dim3(KMP_BLOCK_THREADS), 0, st, elems, carry, n, order, head, flow_of,
                           before32, flow_state);
    ++*launches;
    return hipGetLastError();
}

}  // namespace

size_t kmp_flowbits_order_bytes(uint64_t n, uint64_t n_flows)
{
    if (n == 0) return 0;
    size_t tmp = 0;
    const FbOrder o = {nullptr, nullptr, nullptr, nullptr, nullptr, 0};          /* a size query: rocPRIM looks at no pointer */
    if (fb_sort_run(nullptr, tmp, nullptr, o, n, n_flows, nullptr) != hipSuccess) return 0;
    return fb_order_used(n) + tmp + 256u;
}

hipError_t kmp_launch_flowbits_order(const uint32_t *flow_of, uint64_t n, uint64_t n_flows, uint8_t *order_buf, size_t order_bytes, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    if (n > 0xFFFFFFFEull) return hipErrorInvalidValue;
    const FbOrder o = fb_order(order_buf, n);
    if (order_bytes < o.used) return hipErrorInvalidValue;
    size_t tmp = order_bytes - o.used;
    const hipError_t e = fb_sort_run(o.tmp, tmp, flow_of, o, n, n_flows, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kmp_fb_heads_kernel, dim3(fb_payload_blocks(n + 1u)), dim3(KMP_BLOCK_THREADS), 0, st, o.keys, o.order, n, o.inv, o.head);
    return hipGetLastError();
}

kmp_order_view kmp_flowbits_order_view(const uint8_t *order_buf, uint64_t n)
{
    const FbOrder o = fb_order(const_cast<uint8_t *>(order_buf), n);
    return kmp_order_view{o.order, o.inv, o.keys, o.head};
}

size_t kmp_flowbits_ws_bytes(uint64_t n)
{
    uint64_t elems = fb_pad(n);
    for (uint64_t t = n; t > KMP_SCAN_TILE;) { t = (t + KMP_SCAN_TILE - 1u) / KMP_SCAN_TILE; elems += fb_pad(t); }
    return (size_t)(elems * sizeof(uint2));
}

hipError_t kmp_launch_flowbits_build(const unsigned long long *rule_rows, uint64_t stride, uint64_t n, const uint4 *acting, uint32_t n_act,
                                     const uint32_t *before32, const uint8_t *order_buf, uint8_t *ws, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    if (n > stride * 64u) return hipErrorInvalidValue;
    const FbOrder o = fb_order(const_cast<uint8_t *>(order_buf), n);
    hipLaunchKernelGGL(kmp_fb_build_kernel, dim3(fb_payload_blocks(n)), dim3(KMP_BLOCK_THREADS), 0, st, rule_rows, stride, n, acting, n_act, before32,
                       o.inv, o.head, reinterpret_cast<uint2 *>(ws));
    return hipGetLastError();
}

hipError_t kmp_launch_flowbits_scan(uint64_t n, const uint32_t *flow_of, const uint8_t *order_buf, uint8_t *ws, uint32_t *before32,
                                    uint32_t *flow_state, uint32_t *launches, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    const FbOrder o = fb_order(const_cast<uint8_t *>(order_buf), n);
    uint2 *elems = reinterpret_cast<uint2 *>(ws);
    return fb_scan(elems, n, elems + fb_pad(n), true, o.order, o.head, flow_of, before32, flow_state, launches, st);
}

hipError_t kmp_launch_flowbits_rows(const uint32_t *before32, uint64_t n, uint32_t level_mask, uint64_t stride, unsigned long long *before_rows,
                                    hipStream_t st)
{
    if (n == 0 || level_mask == 0u) return hipSuccess;
    if (n > stride * 64u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kmp_fb_rows_kernel, dim3(fb_payload_blocks(n)), dim3(KMP_BLOCK_THREADS), 0, st, before32, n, level_mask, stride, before_rows);
    return hipGetLastError();
}

hipError_t kmp_launch_flowbits_final(const unsigned long long *rule_rows, const unsigned long long *before_rows, uint64_t stride,
                                     const uint4 *tests, uint32_t n_rules, unsigned long long *alert_rows, unsigned long long *counts,
                                     unsigned long long *any, hipStream_t st)
{
    if (n_rules == 0 || stride == 0) return hipSuccess;
    const uint64_t bx = (stride + KMP_BLOCK_THREADS - 1u) / KMP_BLOCK_THREADS;
    if (bx > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kmp_fb_final_kernel, dim3((uint32_t)bx, std::min(n_rules, FB_FINAL_MAX_BY)), dim3(KMP_BLOCK_THREADS), 0, st, rule_rows,
                       before_rows, stride, tests, n_rules, alert_rows, counts, any);
    return hipGetLastError();
}
