/*
 * kmp_tls.hip -- kmpgpu_tls_locate and kmpgpu_load_tls: where the server name and the ALPN list of the TLS ClientHello in every payload
 * lie, and either of them as a packed arena of its own (kmpgpu.h).  gfx950.
 *
 *   kmp_tls_locate_kernel       one 32-byte kmpgpu_tls_span per payload and, next to it, the 256-bit mask of the ALPN field's positions
 *                               that hold a name's length byte (the gather turns them into ','); hellos, with SNI, with ALPN, truncated
 *   kmp_tls_lengths_kernel      from the spans: the field's length for every payload that has it, 0 or 0xFFFFFFFF ("not in dst", under
 *                               KMPGPU_TLS_ONLY_PRESENT) for any other; the present bitmap, one plain store per word; the stats
 *   kmp_scan_local_kernel, kmp_scan_totals_kernel   of kmp_prep.hip, through kmp_launch_compact_scan
 *   kmp_tls_index_kernel        the new index, and per payload of dst the 16-byte record {source byte address of the field, length,
 *                               payload of the source}
 *   kmp_tls_gather_kernel       the bytes, for both fields
 *
 * The locate.  A lane takes a payload, a wavefront 64 consecutive ones.  The record header, the handshake header and the major byte of
 * the client version are the payload's bytes 0 .. 9, so the first aligned 16-byte unit alone rules out a payload that is no hello: a
 * capture without TLS costs that one load per payload.  The walk (tls_walk) moves forward only and holds one aligned unit in registers
 * (walk_byte, kmp_walk_dev.h, shared with kmp_dns.hip); every position it reads has been compared with E = min(L, end of the hello)
 * first, so a unit is loaded only where it holds a byte in front of E, no load leaves the payload's slot and no byte at or behind L
 * decides anything.  It ends after at most 255 extensions and, inside the one ALPN extension it parses, 256 bytes of names.
 *
 * The lengths kernel's tail, the index and the gather's shape are the compacting skeleton's (group_tail, index_body, gather_runs:
 * kmp_compact_dev.h).  The gather's own part is kmp_dns_gather_kernel's with ',' for '.'.  One gather serves both
 * fields: for the server name the launcher passes no masks, the records' masks stay zero and the separator step changes nothing.
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
using kmp_walk::unit_byte;
using kmp_walk::walk_byte;
using kmp_walk::spread4;

/* grid cap of the locate: rounds past 8 192 groups of 64 payloads, as the HTTP and DNS locates' */
constexpr uint32_t TLS_LOCATE_BLOCKS = 2048;
constexpr uint32_t TLS_EXT_MAX = 255u;           /* extensions that count */
constexpr uint32_t TLS_ALPN_MAX = 256u;          /* bytes of the protocol name list: the separator mask's width */
constexpr uint32_t COMMA4 = 0x2C2C2C2Cu;

/* what the walk finds behind the first unit */
struct TlsHello {
    uint32_t flags, n_ext, sid, n_suites, n_names, sni_off, sni_len, alpn_off, alpn_len;
    uint32_t mk[8];                               /* bit x: byte x of the ALPN field is a separator */
};

/* The hello at p whose first unit passed: L its payload's length, hs the handshake length.  false: the payload is NONE. */
__device__ __forceinline__ bool tls_walk(const uint8_t *p, uint32_t L, uint32_t hs, u32x4 held, TlsHello &h)
{
    uint32_t hu = 0u;
    const uint32_t H = 9u + hs, E = min(L, H);
    auto be16 = [&](uint32_t pos) { const uint32_t hi = walk_byte(p, pos, held, hu); return hi << 8 | walk_byte(p, pos + 1u, held, hu); };
    if (!(43u < E)) return false;
    h.sid = walk_byte(p, 43u, held, hu);
    if (h.sid > 32u) return false;
    uint32_t c = 44u + h.sid;
    if (c + 2u > E) return false;
    const uint32_t cs = be16(c);
    if ((cs & 1u) || cs < 2u) return false;
    h.n_suites = cs >> 1;
    c += 2u + cs;
    if (c >= E) return false;
    const uint32_t cm = walk_byte(p, c, held, hu);
    if (cm < 1u) return false;
    c += 1u + cm;
    if (c == H) return true;                      /* no extensions */
    if (c + 2u > E) return false;
    const uint32_t X = c + 2u + be16(c);
    if (X != H) return false;
    c += 2u;
    const uint32_t Xe = E;                        /* min(X, E), and X == H >= E */
    if (Xe < X) h.flags |= KMPGPU_TLS_TRUNCATED;
    bool sni_seen = false, alpn_seen = false;
    while (c + 4u <= Xe) {
        const uint32_t t = be16(c), n = be16(c + 2u), b = c + 4u;
        if (b + n > X) return false;
        if (b + n > Xe) break;                    /* (a truncated hello's last, partial extension) */
        if (++h.n_ext > TLS_EXT_MAX) return false;
        if (t == 0u && !sni_seen) {
            sni_seen = true;
            if (n < 5u) return false;
            const uint32_t ll = be16(b);
            if (ll + 2u > n) return false;
            if (walk_byte(p, b + 2u, held, hu) != 0u) return false;
            const uint32_t nl = be16(b + 3u);
            if (3u + nl > ll) return false;
            h.flags |= KMPGPU_TLS_HAS_SNI; h.sni_off = b + 5u; h.sni_len = nl;
        } else if (t == 16u && !alpn_seen) {
            alpn_seen = true;
            if (n < 4u) return false;
            const uint32_t ll = be16(b);
            if (ll + 2u != n || ll < 2u) return false;
            if (ll > TLS_ALPN_MAX) {
                h.flags |= KMPGPU_TLS_ALPN_SKIPPED;
            } else {
                const uint32_t end = b + 2u + ll;
                for (uint32_t q = b + 2u; q < end;) {
                    const uint32_t l = walk_byte(p, q, held, hu);
                    if (l < 1u || q + 1u + l > end) return false;
                    if (q > b + 2u) {
                        const uint32_t x = q - (b + 3u);         /* <= 253 */
#pragma unroll
                        for (uint32_t w = 0; w < 8u; ++w) h.mk[w] |= (x >> 5) == w ? 1u << (x & 31u) : 0u;
                    }
                    ++h.n_names;
                    q += 1u + l;
                }
                h.flags |= KMPGPU_TLS_HAS_ALPN; h.alpn_off = b + 3u; h.alpn_len = ll - 1u;
            }
        }
        c = b + n;
    }
    return (h.flags & KMPGPU_TLS_TRUNCATED) || c == X;
}

__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_tls_locate_kernel(const uint8_t *__restrict__ src, const uint64_t *__restrict__ src_off, const uint32_t *__restrict__ src_len, uint64_t n,
                      uint4 *__restrict__ spans, uint4 *__restrict__ masks, unsigned long long *__restrict__ stats)
{
    const uint32_t lane = threadIdx.x & (KMP_WAVE - 1u), wid = threadIdx.x >> 6;
    const uint64_t n_groups = (n + KMP_WAVE - 1u) / KMP_WAVE;
    uint32_t n_hello = 0u, n_sni = 0u, n_alpn = 0u, n_trunc = 0u;      /* per wavefront */
    for (uint64_t r = (uint64_t)blockIdx.x * KMP_BLOCK_WAVES + wid; r < n_groups; r += (uint64_t)gridDim.x * KMP_BLOCK_WAVES) {
        const uint64_t k = r * KMP_WAVE + lane;
        const bool in = k < n;
        const uint32_t L = in ? src_len[k] : 0u;
        const uint64_t so = in ? src_off[k] : 0ull;
        const uint8_t *p = src + so;
        u32x4 v0 = (u32x4)(0u);
        if (L) v0 = load_unit<false>(p);
        const uint32_t rec = unit_byte(v0, 3u) << 8 | unit_byte(v0, 4u);
        const uint32_t hs = unit_byte(v0, 6u) << 16 | unit_byte(v0, 7u) << 8 | unit_byte(v0, 8u);
        /* what the first unit decides: L >= 11 puts all of these bytes in front of the payload's end */
        bool ok = in && L >= 11u && unit_byte(v0, 0u) == 22u && unit_byte(v0, 1u) == 3u && unit_byte(v0, 2u) <= 4u && unit_byte(v0, 5u) == 1u &&
                  unit_byte(v0, 9u) == 3u && rec >= hs + 4u;
        TlsHello h = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u}};
        if (ok) ok = tls_walk(p, L, hs, v0, h);
        uint4 a = make_uint4(0u, 0u, 0u, 0u), b = make_uint4(0u, 0u, 0u, 0u);
        if (ok) {
            a.x = KMPGPU_TLS_CLIENT_HELLO | h.flags << 8 | h.n_ext << 16 | h.sid << 24;
            a.y = (unit_byte(v0, 1u) << 8 | unit_byte(v0, 2u)) | (unit_byte(v0, 9u) << 8 | unit_byte(v0, 10u)) << 16;
            a.z = h.n_suites | h.n_names << 16;
            a.w = hs;
            b.x = h.sni_off; b.y = h.sni_len; b.z = h.alpn_off; b.w = h.alpn_len;
        }
        const bool sep = ok && (h.flags & KMPGPU_TLS_HAS_ALPN);
        if (in) {
            spans[2u * k] = a;
            spans[2u * k + 1u] = b;
            masks[2u * k] = sep ? make_uint4(h.mk[0], h.mk[1], h.mk[2], h.mk[3]) : make_uint4(0u, 0u, 0u, 0u);
            masks[2u * k + 1u] = sep ? make_uint4(h.mk[4], h.mk[5], h.mk[6], h.mk[7]) : make_uint4(0u, 0u, 0u, 0u);
        }
        n_hello += (uint32_t)__popcll(__ballot(ok));
        n_sni += (uint32_t)__popcll(__ballot(ok && (h.flags & KMPGPU_TLS_HAS_SNI)));
        n_alpn += (uint32_t)__popcll(__ballot(sep));
        n_trunc += (uint32_t)__popcll(__ballot(ok && (h.flags & KMPGPU_TLS_TRUNCATED)));
    }
    /* one atomic per BLOCK and counter, as the DNS locate's (one per wavefront was nine tenths of that kernel's time) */
    __shared__ unsigned long long s_stats[KMP_BLOCK_WAVES][4];
    if (lane == 0u) {
        s_stats[wid][0] = n_hello; s_stats[wid][1] = n_sni; s_stats[wid][2] = n_alpn; s_stats[wid][3] = n_trunc;
    }
    __syncthreads();
    if (threadIdx.x < 4u) {
        unsigned long long sum = 0ull;
#pragma unroll
        for (uint32_t w = 0; w < KMP_BLOCK_WAVES; ++w) sum += s_stats[w][threadIdx.x];
        if (sum) atomicAdd(stats + threadIdx.x, sum);
    }
}

/* has: KMPGPU_TLS_HAS_SNI or KMPGPU_TLS_HAS_ALPN, the flag bit of the field asked for */
__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_tls_lengths_kernel(const uint4 *__restrict__ spans, const uint32_t *__restrict__ src_len, uint64_t n, uint32_t has, uint32_t only_present,
                       uint32_t *__restrict__ field_len, unsigned long long *__restrict__ present, unsigned long long *__restrict__ stats)
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
            pres = ((spans[2u * k].x >> 8) & has) != 0u;
            const uint4 b = spans[2u * k + 1u];
            len = pres ? (has == KMPGPU_TLS_HAS_SNI ? b.y : b.w) : 0u;
        }
        group_tail(acc, in, k, r, lane, pres, only_present != 0u, in ? src_len[k] : 0u, len, field_len, present);
    }
    group_sums_flush(acc, lane, stats);
}

/* Payload k of the source is payload j of dst: its slot in the new arena, the field's length, where the field's bytes lie, and k for the
 * separator mask (the scan's payload numbers are 32 bits wide).  A payload without the field has length 0 and its address is not used. */
__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_tls_index_kernel(const uint4 *__restrict__ spans, const uint64_t *__restrict__ src_off, const uint32_t *__restrict__ field_len,
                     const uint64_t *__restrict__ loc_off, const uint32_t *__restrict__ loc_idx, const uint64_t *__restrict__ blk_bytes,
                     const uint32_t *__restrict__ blk_cnt, uint64_t n, uint32_t has, uint64_t *__restrict__ pkt_off,
                     uint32_t *__restrict__ pkt_len, uint4 *__restrict__ recs)
{
    index_body(field_len, loc_off, loc_idx, blk_bytes, blk_cnt, n, pkt_off, pkt_len, recs, [&](uint64_t k, uint32_t l) {
        const uint4 b = spans[2u * k + 1u];
        const uint64_t fs = src_off[k] + (has == KMPGPU_TLS_HAS_SNI ? b.x : b.z);
        return make_uint4((uint32_t)fs, (uint32_t)(fs >> 32), l, (uint32_t)k);
    });
}

struct TlsRec { uint4 rec, m0, m1; };

/* masks: the locate's, for the ALPN field; nullptr for the server name, which has no separators */
template <bool NT>
__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_tls_gather_kernel(const uint8_t *__restrict__ src, const uint64_t *__restrict__ new_off, const uint4 *__restrict__ recs,
                      const uint4 *__restrict__ masks, uint64_t n, uint64_t total, uint32_t run, uint8_t *__restrict__ dst)
{
    __shared__ uint64_t s_src[KMP_BLOCK_WAVES][KMP_WAVE];          /* where payload i's field starts in src */
    __shared__ uint32_t s_len[KMP_BLOCK_WAVES][KMP_WAVE];
    __shared__ uint32_t s_mask[KMP_BLOCK_WAVES][8][KMP_WAVE];      /* word w of payload i's separator mask */
    const uint32_t lane = threadIdx.x & (KMP_WAVE - 1u), wid = threadIdx.x >> 6;
    gather_runs<NT, 2>(new_off, n, total, run, dst,
        [&](uint64_t j, bool in) {
            TlsRec d = {make_uint4(0u, 0u, 0u, 0u), make_uint4(0u, 0u, 0u, 0u), make_uint4(0u, 0u, 0u, 0u)};
            if (in) {
                d.rec = recs[j];
                if (masks && d.rec.z) { d.m0 = masks[2ull * d.rec.w]; d.m1 = masks[2ull * d.rec.w + 1ull]; }
            }
            return d;
        },
        [&](const TlsRec &d) {
            s_src[wid][lane] = ((uint64_t)d.rec.y << 32) | d.rec.x; s_len[wid][lane] = d.rec.z;
            s_mask[wid][0][lane] = d.m0.x; s_mask[wid][1][lane] = d.m0.y; s_mask[wid][2][lane] = d.m0.z; s_mask[wid][3][lane] = d.m0.w;
            s_mask[wid][4][lane] = d.m1.x; s_mask[wid][5][lane] = d.m1.y; s_mask[wid][6][lane] = d.m1.z; s_mask[wid][7][lane] = d.m1.w;
        },
        [&](uint32_t p, uint64_t rel64, uint32_t &) {
            const uint32_t F = s_len[wid][p];
            if (rel64 >= (uint64_t)F) return (u32x4)(0u);            /* (an empty payload's slot: zeros) */
            const uint32_t rel = (uint32_t)rel64;                    /* < 65 536, a multiple of 16 */
            const uint64_t f0 = s_src[wid][p];
            const int32_t fa = (int32_t)(f0 & 15u);                  /* the field in the coordinates of the aligned unit it starts in */
            const uint64_t ua = (f0 - (uint32_t)fa) + rel;           /* 16-byte aligned: the first source unit that holds a byte of it */
            u32x4 v = fetch_piece<NT>(src + ua, fa, fa, fa + (int32_t)min(F - rel, 16u));
            /* the unit's 16 bits; a server name can be longer than the mask is wide, and its mask is zero */
            const uint32_t sep = rel < 256u ? s_mask[wid][(rel >> 5) & 7u][p] >> (rel & 31u) : 0u;
            const uint32_t m0 = spread4(sep), m1 = spread4(sep >> 4), m2 = spread4(sep >> 8), m3 = spread4(sep >> 12);
            v.x = (v.x & ~m0) | (COMMA4 & m0); v.y = (v.y & ~m1) | (COMMA4 & m1);
            v.z = (v.z & ~m2) | (COMMA4 & m2); v.w = (v.w & ~m3) | (COMMA4 & m3);
            return v;
        });
}

uint32_t has_bit(int field) { return field == KMPGPU_TLS_SNI ? KMPGPU_TLS_HAS_SNI : KMPGPU_TLS_HAS_ALPN; }

}  // namespace

hipError_t kmp_launch_tls_locate(const uint8_t *src_arena, const uint64_t *src_off, const uint32_t *src_len, uint64_t n, void *spans,
                                 void *masks, unsigned long long *stats, hipStream_t st)
{
    static_assert(sizeof(kmpgpu_tls_span) == 32, "kmpgpu_tls_span is two 16-byte units");
    if (n == 0) return hipSuccess;
    const uint64_t groups = (n + KMP_WAVE - 1) / KMP_WAVE;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((groups + KMP_BLOCK_WAVES - 1) / KMP_BLOCK_WAVES, TLS_LOCATE_BLOCKS);
    hipLaunchKernelGGL(kmp_tls_locate_kernel, dim3(blocks), dim3(KMP_BLOCK_THREADS), 0, st, src_arena, src_off, src_len, n,
                       reinterpret_cast<uint4 *>(spans), reinterpret_cast<uint4 *>(masks), stats);
    return hipGetLastError();
}

hipError_t kmp_launch_tls_lengths(const void *spans, const uint32_t *src_len, uint64_t n, int field, bool only_present, uint8_t *ws,
                                  unsigned long long *present, unsigned long long *stats, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(kmp_tls_lengths_kernel, dim3(kmp_group_blocks(n)), dim3(KMP_BLOCK_THREADS), 0, st, reinterpret_cast<const uint4 *>(spans), src_len, n,
                       has_bit(field), only_present ? 1u : 0u, kmp_compact_ws(ws, n).len, present, stats);
    return hipGetLastError();
}

hipError_t kmp_launch_tls_index(const void *spans, const uint64_t *src_off, uint64_t n, int field, uint8_t *ws, uint64_t n_dst,
                                uint64_t *pkt_off, uint32_t *pkt_len, void *recs, hipStream_t st)
{
    if (n == 0 || n_dst == 0) return hipSuccess;
    const kmp_compact_view w = kmp_compact_ws(ws, n);
    hipLaunchKernelGGL(kmp_tls_index_kernel, dim3(kmp_item_blocks(n)), dim3(KMP_BLOCK_THREADS), 0, st, reinterpret_cast<const uint4 *>(spans), src_off,
                       w.len, w.loc_off, w.loc_idx, w.blk_bytes, w.blk_cnt, n, has_bit(field), pkt_off, pkt_len, reinterpret_cast<uint4 *>(recs));
    return hipGetLastError();
}

hipError_t kmp_launch_tls_gather(const uint8_t *src_arena, const uint64_t *pkt_off, const void *recs, const void *masks, int field,
                                 uint64_t n_dst, uint64_t total_bytes, uint8_t *arena, bool nontemporal, hipStream_t st)
{
    if (n_dst == 0) return hipSuccess;
    const kmp_run_shape rs = kmp_run_shape_of(n_dst, total_bytes);
    hipLaunchKernelGGL(nontemporal ? kmp_tls_gather_kernel<true> : kmp_tls_gather_kernel<false>, dim3(rs.blocks), dim3(KMP_BLOCK_THREADS), 0, st,
                       src_arena, pkt_off, (const uint4 *)recs, field == KMPGPU_TLS_ALPN ? (const uint4 *)masks : nullptr, n_dst, total_bytes,
                       rs.run, arena);
    return hipGetLastError();
}
