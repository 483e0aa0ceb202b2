/*
 * kmp_dns.hip -- kmpgpu_dns_locate and kmpgpu_load_dns: where the first question of the DNS message in every payload lies, and its name in
 * dotted form as a packed arena of its own (kmpgpu.h).  gfx950.
 *
 *   kmp_dns_locate_kernel       one 32-byte kmpgpu_dns_span per payload and, next to it, the 256-bit mask of the name's positions that
 *                               hold a label's length byte (the gather turns them into '.'); queries, responses, root names, name bytes
 *   kmp_dns_lengths_kernel      from the spans: name_len of every payload that is a message, or 0xFFFFFFFF ("not in dst") for any other
 *                               under KMPGPU_DNS_ONLY_PRESENT; the present bitmap, one plain store per word; the stats
 *   kmp_scan_local_kernel, kmp_scan_totals_kernel   of kmp_prep.hip, through kmp_launch_compact_scan
 *   kmp_dns_index_kernel        the new index, and per payload of dst the 16-byte record {source byte address of the name, length,
 *                               payload of the source}
 *   kmp_dns_gather_kernel       the bytes
 *
 * The locate.  A lane takes a payload, a wavefront 64 consecutive ones.  The first aligned 16-byte unit holds the header, QDCOUNT and the
 * first length byte whether or not a 2-byte length stands in front, so it alone rules out a payload that is too short, asks nothing or
 * starts its name with a byte above 63: a capture without DNS costs that one load per payload.  The walk over the labels moves forward
 * only and holds one aligned unit in registers: a length byte comes out of the held unit by selects and shifts, and the next unit is
 * loaded when the walk leaves the held one.  A unit is loaded only where it holds a byte in front of the payload's end, so no load leaves
 * the payload's slot.  A name is at most 255 bytes on the wire, so the walk ends after at most 127 labels.
 *
 * The lengths kernel's tail, the index and the gather's shape are the compacting skeleton's (group_tail, index_body, gather_runs:
 * kmp_compact_dev.h).  The gather's own part is kmp_fields_gather_kernel's: a destination unit is built from the one or
 * two ALIGNED source units that hold its bytes (fetch_piece, kmp_piece_dev.h) and cleared behind the name's end; then the 16 bits of the
 * separator mask that belong to the unit put '.' over the length bytes, in registers, before the store.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "kmpgpu.h"
#include "kmp_device.h"
#include "kmp_launch.h"
#include "kmp_piece_dev.h"
#include "kmp_walk_dev.h"
#include "kmp_compact_dev.h"

namespace {

using namespace kmp_unit;     /* kmp_compact_dev.h: group_tail, index_body, gather_runs; kmp_unit_dev.h: the unit */
using kmp_piece::fetch_piece;
using kmp_walk::unit_byte;      /* kmp_walk_dev.h: the held unit of a forward walk, shared with kmp_tls.hip */
using kmp_walk::walk_byte;
using kmp_walk::spread4;

/* grid cap of the locate: rounds past 8 192 groups of 64 payloads, as the HTTP locate's */
constexpr uint32_t DNS_LOCATE_BLOCKS = 2048;
constexpr uint32_t DNS_NAME_MAX = 255u;          /* wire bytes of a name, its closing 0x00 included */
constexpr uint32_t DOT4 = 0x2E2E2E2Eu;

/* B: the bytes in front of the message (0, or 2 under KMPGPU_DNS_TCP_PREFIX) */
template <uint32_t B>
__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_dns_locate_kernel(const uint8_t *__restrict__ src, const uint64_t *__restrict__ src_off, const uint32_t *__restrict__ src_len, uint64_t n,
                      uint4 *__restrict__ spans, uint4 *__restrict__ masks, unsigned long long *__restrict__ stats)
{
    const uint32_t lane = threadIdx.x & (KMP_WAVE - 1u), wid = threadIdx.x >> 6;
    const uint64_t n_groups = (n + KMP_WAVE - 1u) / KMP_WAVE;
    uint32_t n_query = 0u, n_resp = 0u, n_root = 0u;            /* per wavefront */
    unsigned long long name_bytes = 0ull;                       /* per lane */
    for (uint64_t r = (uint64_t)blockIdx.x * KMP_BLOCK_WAVES + wid; r < n_groups; r += (uint64_t)gridDim.x * KMP_BLOCK_WAVES) {
        const uint64_t k = r * KMP_WAVE + lane;
        const bool in = k < n;
        const uint32_t L = in ? src_len[k] : 0u;
        const uint64_t so = in ? src_off[k] : 0ull;
        const uint8_t *p = src + so;
        u32x4 v0 = (u32x4)(0u);
        if (L) v0 = load_unit<false>(p);
        const uint32_t M = L >= B ? L - B : 0u;
        const uint32_t qd = unit_byte(v0, B + 4u) << 8 | unit_byte(v0, B + 5u);
        /* what the first unit decides: M >= 17 puts all of these bytes in front of the payload's end */
        bool ok = in && M >= 17u && qd >= 1u && unit_byte(v0, B + 12u) <= 63u;
        uint32_t mk[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};      /* bit x: byte x of the name is a separator */
        uint32_t i = 12u, n_labels = 0u, qtype = 0u, qclass = 0u;
        if (ok) {
            u32x4 held = v0;
            uint32_t hu = 0u;
            for (;;) {
                if (i >= M) { ok = false; break; }
                const uint32_t c = walk_byte(p, B + i, held, hu);
                if (c == 0u) break;
                /* a pointer or a reserved label type; a label that leaves the payload; a name longer than 255 bytes on the wire */
                if (c > 63u || i + 1u + c > M || i + 1u + c + 1u - 12u > DNS_NAME_MAX) { ok = false; break; }
                if (i > 12u) {
                    const uint32_t x = i - 13u;                  /* <= 253 */
#pragma unroll
                    for (uint32_t w = 0; w < 8u; ++w) mk[w] |= (x >> 5) == w ? 1u << (x & 31u) : 0u;
                }
                ++n_labels;
                i += 1u + c;
            }
            if (ok && i + 5u > M) ok = false;                    /* QTYPE and QCLASS lie inside the payload */
            if (ok) {
                qtype = walk_byte(p, B + i + 1u, held, hu) << 8;
                qtype |= walk_byte(p, B + i + 2u, held, hu);
                qclass = walk_byte(p, B + i + 3u, held, hu) << 8;
                qclass |= walk_byte(p, B + i + 4u, held, hu);
            }
        }
        uint4 a = make_uint4(0u, 0u, 0u, 0u), b = make_uint4(0u, 0u, 0u, 0u);
        const uint32_t name_len = ok && i > 13u ? i - 13u : 0u;
        bool resp = false;
        if (ok) {
            const uint32_t id = unit_byte(v0, B + 0u) << 8 | unit_byte(v0, B + 1u);
            const uint32_t fl = unit_byte(v0, B + 2u) << 8 | unit_byte(v0, B + 3u);
            const uint32_t an = unit_byte(v0, B + 6u) << 8 | unit_byte(v0, B + 7u);
            const uint32_t ns = unit_byte(v0, B + 8u) << 8 | unit_byte(v0, B + 9u);
            const uint32_t ar = unit_byte(v0, B + 10u) << 8 | unit_byte(v0, B + 11u);
            resp = (fl & 0x8000u) != 0u;
            a.x = (resp ? KMPGPU_DNS_RESPONSE : KMPGPU_DNS_QUERY) | n_labels << 8 | fl << 16;
            a.y = id | qtype << 16;
            a.z = qclass | qd << 16;
            a.w = an | ns << 16;
            b.x = ar;
            b.y = B + 13u; b.z = name_len; b.w = B + i + 5u;
        }
        if (in) {
            spans[2u * k] = a;
            spans[2u * k + 1u] = b;
            masks[2u * k] = ok ? make_uint4(mk[0], mk[1], mk[2], mk[3]) : make_uint4(0u, 0u, 0u, 0u);
            masks[2u * k + 1u] = ok ? make_uint4(mk[4], mk[5], mk[6], mk[7]) : make_uint4(0u, 0u, 0u, 0u);
        }
        n_query += (uint32_t)__popcll(__ballot(ok && !resp));
        n_resp += (uint32_t)__popcll(__ballot(ok && resp));
        n_root += (uint32_t)__popcll(__ballot(ok && i == 12u));
        name_bytes += name_len;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) name_bytes += __shfl_xor(name_bytes, o);
    /* one atomic per BLOCK and counter: the atomics of all wavefronts meet on one cache line and are carried out one after the other,
     * ~12 ns each -- with one per wavefront and counter they were nine tenths of the kernel's time over a capture of DNS messages */
    __shared__ unsigned long long s_stats[KMP_BLOCK_WAVES][4];
    if (lane == 0u) {
        s_stats[wid][0] = n_query; s_stats[wid][1] = n_resp; s_stats[wid][2] = n_root; s_stats[wid][3] = name_bytes;
    }
    __syncthreads();
    if (threadIdx.x < 4u) {
        unsigned long long sum = 0ull;
#pragma unroll
        for (uint32_t w = 0; w < KMP_BLOCK_WAVES; ++w) sum += s_stats[w][threadIdx.x];
        if (sum) atomicAdd(stats + threadIdx.x, sum);
    }
}

__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_dns_lengths_kernel(const uint4 *__restrict__ spans, const uint32_t *__restrict__ src_len, uint64_t n, uint32_t only_present,
                       uint32_t *__restrict__ name_len, unsigned long long *__restrict__ present, unsigned long long *__restrict__ stats)
{
    const uint32_t lane = threadIdx.x & (KMP_WAVE - 1u), wid = threadIdx.x >> 6;
    const uint64_t n_groups = (n + KMP_WAVE - 1u) / KMP_WAVE;
    GroupSums acc = {0ull, 0ull, 0ull};
    for (uint64_t r = (uint64_t)blockIdx.x * KMP_BLOCK_WAVES + wid; r < n_groups; r += (uint64_t)gridDim.x * KMP_BLOCK_WAVES) {
        const uint64_t k = r * KMP_WAVE + lane;
        const bool in = k < n;
        uint32_t len = 0u;
        bool pres = false;
        if (in) {
            pres = (spans[2u * k].x & 0xFFu) != KMPGPU_DNS_NONE;
            len = pres ? spans[2u * k + 1u].z : 0u;
        }
        group_tail(acc, in, k, r, lane, pres, only_present != 0u, in ? src_len[k] : 0u, len, name_len, present);
    }
    group_sums_flush(acc, lane, stats);
}

/* Payload k of the source is payload j of dst: its slot in the new arena, the name's length, where the name's bytes lie, and k for the
 * separator mask (the scan's payload numbers are 32 bits wide) */
__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_dns_index_kernel(const uint4 *__restrict__ spans, const uint64_t *__restrict__ src_off, const uint32_t *__restrict__ name_len,
                     const uint64_t *__restrict__ loc_off, const uint32_t *__restrict__ loc_idx, const uint64_t *__restrict__ blk_bytes,
                     const uint32_t *__restrict__ blk_cnt, uint64_t n, uint64_t *__restrict__ pkt_off, uint32_t *__restrict__ pkt_len,
                     uint4 *__restrict__ recs)
{
    index_body(name_len, loc_off, loc_idx, blk_bytes, blk_cnt, n, pkt_off, pkt_len, recs, [&](uint64_t k, uint32_t l) {
        const uint64_t fs = src_off[k] + spans[2u * k + 1u].y;
        return make_uint4((uint32_t)fs, (uint32_t)(fs >> 32), l, (uint32_t)k);
    });
}

struct DnsRec { uint4 rec, m0, m1; };

template <bool NT>
__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_dns_gather_kernel(const uint8_t *__restrict__ src, const uint64_t *__restrict__ new_off, const uint4 *__restrict__ recs,
                      const uint4 *__restrict__ masks, uint64_t n, uint64_t total, uint32_t run, uint8_t *__restrict__ dst)
{
    __shared__ uint64_t s_src[KMP_BLOCK_WAVES][KMP_WAVE];          /* where payload i's name starts in src */
    __shared__ uint32_t s_len[KMP_BLOCK_WAVES][KMP_WAVE];
    __shared__ uint32_t s_mask[KMP_BLOCK_WAVES][8][KMP_WAVE];      /* word w of payload i's separator mask */
    const uint32_t lane = threadIdx.x & (KMP_WAVE - 1u), wid = threadIdx.x >> 6;
    gather_runs<NT, 2>(new_off, n, total, run, dst,
        [&](uint64_t j, bool in) {
            DnsRec d = {make_uint4(0u, 0u, 0u, 0u), make_uint4(0u, 0u, 0u, 0u), make_uint4(0u, 0u, 0u, 0u)};
            if (in) {
                d.rec = recs[j];
                if (d.rec.z) { d.m0 = masks[2ull * d.rec.w]; d.m1 = masks[2ull * d.rec.w + 1ull]; }
            }
            return d;
        },
        [&](const DnsRec &d) {
            s_src[wid][lane] = ((uint64_t)d.rec.y << 32) | d.rec.x; s_len[wid][lane] = d.rec.z;
            s_mask[wid][0][lane] = d.m0.x; s_mask[wid][1][lane] = d.m0.y; s_mask[wid][2][lane] = d.m0.z; s_mask[wid][3][lane] = d.m0.w;
            s_mask[wid][4][lane] = d.m1.x; s_mask[wid][5][lane] = d.m1.y; s_mask[wid][6][lane] = d.m1.z; s_mask[wid][7][lane] = d.m1.w;
        },
        [&](uint32_t p, uint64_t rel64, uint32_t &) {
            const uint32_t F = s_len[wid][p];
            if (rel64 >= (uint64_t)F) return (u32x4)(0u);            /* (an empty payload's slot: zeros) */
            const uint32_t rel = (uint32_t)rel64;                    /* < 256, a multiple of 16 */
            const uint64_t f0 = s_src[wid][p];
            const int32_t fa = (int32_t)(f0 & 15u);                  /* the name in the coordinates of the aligned unit it starts in */
            const uint64_t ua = (f0 - (uint32_t)fa) + rel;           /* 16-byte aligned: the first source unit that holds a byte of it */
            u32x4 v = fetch_piece<NT>(src + ua, fa, fa, fa + (int32_t)min(F - rel, 16u));
            const uint32_t sep = s_mask[wid][rel >> 5][p] >> (rel & 31u);            /* the unit's 16 bits */
            const uint32_t m0 = spread4(sep), m1 = spread4(sep >> 4), m2 = spread4(sep >> 8), m3 = spread4(sep >> 12);
            v.x = (v.x & ~m0) | (DOT4 & m0); v.y = (v.y & ~m1) | (DOT4 & m1);
            v.z = (v.z & ~m2) | (DOT4 & m2); v.w = (v.w & ~m3) | (DOT4 & m3);
            return v;
        });
}

}  // namespace

hipError_t kmp_launch_dns_locate(const uint8_t *src_arena, const uint64_t *src_off, const uint32_t *src_len, uint64_t n, bool tcp_prefix,
                                 void *spans, void *masks, unsigned long long *stats, hipStream_t st)
{
    static_assert(sizeof(kmpgpu_dns_span) == 32, "kmpgpu_dns_span is two 16-byte units");
    if (n == 0) return hipSuccess;
    const uint64_t groups = (n + KMP_WAVE - 1) / KMP_WAVE;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((groups + KMP_BLOCK_WAVES - 1) / KMP_BLOCK_WAVES, DNS_LOCATE_BLOCKS);
    hipLaunchKernelGGL(tcp_prefix ? kmp_dns_locate_kernel<2u> : kmp_dns_locate_kernel<0u>, dim3(blocks), dim3(KMP_BLOCK_THREADS), 0, st,
                       src_arena, src_off, src_len, n, reinterpret_cast<uint4 *>(spans), reinterpret_cast<uint4 *>(masks), stats);
    return hipGetLastError();
}

hipError_t kmp_launch_dns_lengths(const void *spans, const uint32_t *src_len, uint64_t n, bool only_present, uint8_t *ws,
                                  unsigned long long *present, unsigned long long *stats, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(kmp_dns_lengths_kernel, dim3(kmp_group_blocks(n)), dim3(KMP_BLOCK_THREADS), 0, st, reinterpret_cast<const uint4 *>(spans), src_len, n,
                       only_present ? 1u : 0u, kmp_compact_ws(ws, n).len, present, stats);
    return hipGetLastError();
}

hipError_t kmp_launch_dns_index(const void *spans, const uint64_t *src_off, uint64_t n, uint8_t *ws, uint64_t n_dst, uint64_t *pkt_off,
                                uint32_t *pkt_len, void *recs, hipStream_t st)
{
    if (n == 0 || n_dst == 0) return hipSuccess;
    const kmp_compact_view w = kmp_compact_ws(ws, n);
    hipLaunchKernelGGL(kmp_dns_index_kernel, dim3(kmp_item_blocks(n)), dim3(KMP_BLOCK_THREADS), 0, st, reinterpret_cast<const uint4 *>(spans), src_off,
                       w.len, w.loc_off, w.loc_idx, w.blk_bytes, w.blk_cnt, n, pkt_off, pkt_len, reinterpret_cast<uint4 *>(recs));
    return hipGetLastError();
}

hipError_t kmp_launch_dns_gather(const uint8_t *src_arena, const uint64_t *pkt_off, const void *recs, const void *masks, uint64_t n_dst,
                                 uint64_t total_bytes, uint8_t *arena, bool nontemporal, hipStream_t st)
{
    if (n_dst == 0) return hipSuccess;
    const kmp_run_shape rs = kmp_run_shape_of(n_dst, total_bytes);
    hipLaunchKernelGGL(nontemporal ? kmp_dns_gather_kernel<true> : kmp_dns_gather_kernel<false>, dim3(rs.blocks), dim3(KMP_BLOCK_THREADS), 0, st,
                       src_arena, pkt_off, (const uint4 *)recs, (const uint4 *)masks, n_dst, total_bytes, rs.run, arena);
    return hipGetLastError();
}
