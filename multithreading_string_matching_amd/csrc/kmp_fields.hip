/*
 * kmp_fields.hip -- kmpgpu_http_locate and kmpgpu_load_fields: where the HTTP message at the start of every payload keeps its method, URI,
 * status, headers and body, and one of those fields of every payload as a packed arena of its own (kmpgpu.h).  gfx950.
 *
 *   kmp_http_locate_kernel      one 32-byte kmpgpu_http_span per payload; requests, responses, blank lines and the bytes looked at
 *   kmp_fields_lengths_kernel   from the spans: field_len[k] of the asked field, or 0xFFFFFFFF ("not in dst") for an absent one under
 *                               KMPGPU_FIELDS_ONLY_PRESENT; the present bitmap, one plain store per word; the stats
 *   kmp_scan_local_kernel, kmp_scan_totals_kernel   of kmp_prep.hip, through kmp_launch_compact_scan
 *   kmp_fields_index_kernel     the new index, and per payload of dst the 16-byte record {source byte address of the field, length}
 *   kmp_fields_gather_kernel    the bytes
 *
 * The locate.  Every term of the definition is "the smallest index with a local property", so nothing walks a payload byte by byte.  A
 * wavefront takes 64 consecutive payloads.  Lane i loads the first 16-byte unit of payload i and rules the payload out from it alone
 * where it neither starts with "HTTP/" nor with 1..15 upper-case letters and a ' ': a capture without HTTP costs that one load per
 * payload.  The remaining payloads are taken one after the other (a scalar loop over the ballot) by the whole wavefront, 1 KiB per step:
 * 64 aligned 16-byte loads, per lane the 16-bit masks of '\n', '\r' and ' ' among the bytes inside the payload, and the first position
 * of a property from a ballot, the first lane's number and that lane's mask.  The blank-line test needs the two bytes behind a '\n': the
 * masks of the lane behind come through a lane shift, and lane 63 loads the step's next unit where its own unit has a '\n' in its last
 * two bytes.  A byte at or behind the payload's end has no bit in any mask.  A payload is left at the step that holds its blank line
 * (one step for a typical request), or the end of its start line where that line makes it no message after all.
 *
 * The lengths kernel's tail, the index and the gather's shape are the compacting skeleton's (group_tail, index_body, gather_runs:
 * kmp_compact_dev.h).  The gather's own part is kmp_seam_gather_kernel's with one piece per payload: a destination unit is
 * built from the one or two ALIGNED source units that hold its bytes (fetch_piece, kmp_piece_dev.h), cleared behind the field's end in
 * registers.  An aligned unit that holds a byte of a payload lies inside that payload's slot, so no load leaves the slot; a field that
 * starts on a multiple of 16 (METHOD always does) is one load per unit.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "kmpgpu.h"
#include "kmp_device.h"
#include "kmp_launch.h"
#include "kmp_piece_dev.h"
#include "kmp_compact_dev.h"

namespace {

using namespace kmp_unit;     /* kmp_compact_dev.h: group_tail, index_body, gather_runs; kmp_unit_dev.h: the unit, byte classes */
using kmp_piece::fetch_piece;

constexpr uint32_t FLD_NONE = 0xFFFFFFFFu;
constexpr uint32_t FLD_STEP = 1024u;             /* bytes of a payload the locate takes per step: 64 lanes x 16 */
/* grid cap of the locate: rounds past 8 192 groups of 64 payloads.  8 wavefronts per SIMD: a wavefront has one step of 1 KiB in flight and
 * waits for it before it knows where to go on, so it is the number of wavefronts that hides the latency */
constexpr uint32_t FLD_LOCATE_BLOCKS = 2048;

/* ---- byte classes of a dword, 0x80 in every byte of the class (eq_bytes, bits4, eq16: kmp_unit_dev.h) ---- */
__device__ __forceinline__ uint32_t upper_bytes(uint32_t w)
{
    const uint32_t lo7 = w & 0x7F7F7F7Fu;
    return (lo7 + 0x3F3F3F3Fu) & ~(lo7 + 0x25252525u) & ~w & 0x80808080u;        /* 0x41 <= b <= 0x5A */
}
__device__ __forceinline__ uint32_t upper16(u32x4 v)
{
    return bits4(upper_bytes(v.x)) | bits4(upper_bytes(v.y)) << 4 | bits4(upper_bytes(v.z)) << 8 | bits4(upper_bytes(v.w)) << 12;
}
constexpr uint32_t LF4 = 0x0A0A0A0Au, CR4 = 0x0D0D0D0Du, SP4 = 0x20202020u;
constexpr uint32_t HTTP4 = 0x50545448u;          /* "HTTP", little-endian */

/* The smallest position of a step (lane l holds the positions 16 l .. 16 l + 15 as the bits of m16) that has its bit set; the same
 * value in every lane.  All 64 lanes take part. */
__device__ __forceinline__ uint32_t first_pos(uint32_t m16)
{
    const unsigned long long b = __ballot(m16 != 0u);
    if (!b) return FLD_NONE;
    const uint32_t l = (uint32_t)__builtin_ctzll(b);
    const uint32_t m = (uint32_t)__builtin_amdgcn_readlane((int)m16, (int)l);
    return 16u * l + (uint32_t)__builtin_ctz(m);
}
/* the bit of position x (0 .. 1023) of a step */
__device__ __forceinline__ uint32_t bit_at(uint32_t m16, uint32_t x)
{
    return ((uint32_t)__builtin_amdgcn_readlane((int)m16, (int)(x >> 4)) >> (x & 15u)) & 1u;
}

__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_http_locate_kernel(const uint8_t *__restrict__ src, const uint64_t *__restrict__ src_off, const uint32_t *__restrict__ src_len, uint64_t n,
                       uint4 *__restrict__ spans, unsigned long long *__restrict__ stats)
{
    const uint32_t lane = threadIdx.x & (KMP_WAVE - 1u), wid = threadIdx.x >> 6;
    const uint64_t n_groups = (n + KMP_WAVE - 1u) / KMP_WAVE;
    unsigned long long lane_bytes = 0ull, wave_bytes = 0ull;    /* per lane: the payloads ruled out; per wavefront: the ones read on */
    uint32_t n_req = 0u, n_resp = 0u, n_blank = 0u;             /* per wavefront */
    for (uint64_t r = (uint64_t)blockIdx.x * KMP_BLOCK_WAVES + wid; r < n_groups; r += (uint64_t)gridDim.x * KMP_BLOCK_WAVES) {
        const uint64_t k = r * KMP_WAVE + lane;
        const bool in = k < n;
        const uint32_t L = in ? src_len[k] : 0u;
        const uint64_t so = in ? src_off[k] : 0ull;
        u32x4 v0 = (u32x4)(0u);
        if (L) v0 = load_unit<false>(src + so);
        const uint32_t valid0 = valid_bits(L);
        const bool resp = L >= 5u && v0.x == HTTP4 && (v0.y & 0xFFu) == 0x2Fu;
        const uint32_t sp0 = eq16(v0, SP4) & valid0, up0 = upper16(v0) & valid0;
        const uint32_t s0 = sp0 ? (uint32_t)__builtin_ctz(sp0) : 0u;
        const bool req = s0 >= 1u && (up0 & ((1u << s0) - 1u)) == (1u << s0) - 1u;
        const bool cand = in && (resp || req);
        if (in && !cand) {
            spans[2u * k] = make_uint4(0u, 0u, 0u, 0u);
            spans[2u * k + 1u] = make_uint4(0u, 0u, 0u, 0u);
            lane_bytes += min(L, 16u);
        }
        unsigned long long todo = __ballot(cand);
        while (todo) {
            const uint32_t q = (uint32_t)__builtin_ctzll(todo);
            todo &= todo - 1ull;
            const uint32_t Lq = (uint32_t)__builtin_amdgcn_readlane((int)L, (int)q);
            const uint64_t soq = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)so, (int)q) |
                                 (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(so >> 32), (int)q) << 32;
            const bool respq = __builtin_amdgcn_readlane((int)resp, (int)q) != 0;
            const uint8_t *p = src + soq;
            uint32_t e = FLD_NONE, s1 = FLD_NONE, s2 = FLD_NONE, bl = FLD_NONE, form = 0u;
            uint32_t prev_cr = 0u, cr_before_e = 0u, last_cr = 0u, scanned = 0u;
            for (uint64_t sb = 0; sb < Lq; sb += FLD_STEP) {
                const uint64_t pos = sb + 16u * lane;
                const bool act = pos < Lq;
                u32x4 v = (u32x4)(0u);
                if (act) v = load_unit<false>(p + pos);
                const uint32_t valid = act ? valid_bits((uint32_t)min((uint64_t)Lq - pos, (uint64_t)16u)) : 0u;
                const uint32_t lf = eq16(v, LF4) & valid, cr = eq16(v, CR4) & valid;
                scanned = (uint32_t)min((uint64_t)Lq, sb + FLD_STEP);
                if (e == FLD_NONE) {
                    /* the start line: its end, and the first two ' ' in front of it */
                    uint32_t sp = eq16(v, SP4) & valid;
                    const uint32_t fe = first_pos(lf);
                    if (fe != FLD_NONE) {
                        const uint32_t b0 = 16u * lane;
                        sp &= fe <= b0 ? 0u : fe >= b0 + 16u ? 0xFFFFu : (1u << (fe - b0)) - 1u;
                    }
                    if (s1 == FLD_NONE) {
                        const uint32_t f = first_pos(sp);
                        if (f != FLD_NONE) {
                            s1 = (uint32_t)sb + f;
                            if (lane == (f >> 4)) sp &= ~(1u << (f & 15u));
                        }
                    }
                    if (s1 != FLD_NONE && s2 == FLD_NONE) {
                        const uint32_t f = first_pos(sp);
                        if (f != FLD_NONE) s2 = (uint32_t)sb + f;
                    }
                    if (fe != FLD_NONE) {
                        e = (uint32_t)sb + fe;
                        cr_before_e = fe ? bit_at(cr, fe - 1u) : prev_cr;
                    }
                }
                prev_cr = bit_at(cr, FLD_STEP - 1u);
                if (sb + FLD_STEP >= Lq) last_cr = bit_at(cr, (uint32_t)(Lq - 1u - sb));
                /* the blank line: a '\n' with "\n" or "\r\n" behind it, inside the payload */
                uint32_t nlf = __shfl_down(lf, 1), ncr = __shfl_down(cr, 1);
                if (lane == KMP_WAVE - 1u) {
                    nlf = 0u; ncr = 0u;
                    if ((lf & 0xC000u) && pos + 16u < Lq) {
                        const u32x4 nv = load_unit<false>(p + pos + 16u);
                        const uint32_t nvalid = valid_bits((uint32_t)min((uint64_t)Lq - pos - 16u, (uint64_t)16u));
                        nlf = eq16(nv, LF4) & nvalid; ncr = eq16(nv, CR4) & nvalid;
                    }
                }
                const uint32_t lfx = lf | (nlf & 3u) << 16, crx = cr | (ncr & 3u) << 16;
                const uint32_t blank = lf & ((lfx >> 1) | ((crx >> 1) & (lfx >> 2)));
                const uint32_t fb = first_pos(blank);
                if (fb != FLD_NONE) {
                    bl = (uint32_t)sb + fb;
                    form = bit_at(lfx >> 1, fb) ? 2u : 3u;             /* what lies between the '\n' and the body's first byte, + 1 */
                    break;
                }
                if (e != FLD_NONE && !respq) {
                    /* a start line that is no request line after all: nothing of this payload is looked at further */
                    const uint32_t ep = cr_before_e ? e - 1u : e;
                    if (!(s1 != FLD_NONE && s1 + 1u < ep)) break;
                }
            }
            const bool has_lf = e != FLD_NONE;
            if (!has_lf) { e = Lq; cr_before_e = last_cr; }
            const uint32_t ep = cr_before_e ? e - 1u : e;
            const bool has_s1 = s1 != FLD_NONE && s1 + 1u < ep;
            if (s1 != FLD_NONE && s2 == FLD_NONE) s2 = ep;
            const uint32_t kind = respq ? KMPGPU_HTTP_RESPONSE : has_s1 ? KMPGPU_HTTP_REQUEST : KMPGPU_HTTP_NONE;
            uint4 a = make_uint4(0u, 0u, 0u, 0u), b = make_uint4(0u, 0u, 0u, 0u);
            if (kind != KMPGPU_HTTP_NONE) {
                const bool has_blank = bl != FLD_NONE;
                const uint32_t flags = (has_lf ? KMPGPU_HTTP_HAS_LF : 0u) | (has_blank ? KMPGPU_HTTP_HAS_BLANK : 0u) | (has_s1 ? KMPGPU_HTTP_HAS_TOKEN : 0u);
                a.x = kind | flags << 8 | (kind == KMPGPU_HTTP_REQUEST ? s1 : 0u) << 16;
                if (has_s1) { a.y = s1 + 1u; a.z = s2 - s1 - 1u; }
                if (has_lf) { a.w = e + 1u; b.x = (has_blank ? bl + 1u : Lq) - (e + 1u); }
                if (has_blank) { b.y = bl + form; b.z = Lq - (bl + form); }
                n_req += kind == KMPGPU_HTTP_REQUEST ? 1u : 0u;
                n_resp += kind == KMPGPU_HTTP_RESPONSE ? 1u : 0u;
                n_blank += has_blank ? 1u : 0u;
            }
            wave_bytes += scanned;
            if (lane == 0u) {
                const uint64_t kq = r * KMP_WAVE + q;
                spans[2u * kq] = a;
                spans[2u * kq + 1u] = b;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) lane_bytes += __shfl_xor(lane_bytes, o);
    if (lane == 0u) {
        if (n_req) atomicAdd(stats + 0, (unsigned long long)n_req);
        if (n_resp) atomicAdd(stats + 1, (unsigned long long)n_resp);
        if (n_blank) atomicAdd(stats + 2, (unsigned long long)n_blank);
        if (lane_bytes + wave_bytes) atomicAdd(stats + 3, lane_bytes + wave_bytes);
    }
}

/* One field of a payload from its span: present or not, where it starts in the payload and how long it is. */
__device__ __forceinline__ bool field_of(uint4 a, uint4 b, uint32_t field, uint32_t *off, uint32_t *len)
{
    const uint32_t kind = a.x & 0xFFu, flags = (a.x >> 8) & 0xFFu;
    bool present = false;
    uint32_t o = 0u, l = 0u;
    switch (field) {
    case KMPGPU_FIELD_METHOD:  present = kind == KMPGPU_HTTP_REQUEST; l = a.x >> 16; break;
    case KMPGPU_FIELD_RAW_URI: present = kind == KMPGPU_HTTP_REQUEST; o = a.y; l = a.z; break;
    case KMPGPU_FIELD_STATUS:  present = kind == KMPGPU_HTTP_RESPONSE && (flags & KMPGPU_HTTP_HAS_TOKEN); o = a.y; l = a.z; break;
    case KMPGPU_FIELD_HEADERS: present = kind != KMPGPU_HTTP_NONE && (flags & KMPGPU_HTTP_HAS_LF); o = a.w; l = b.x; break;
    default:                   present = kind != KMPGPU_HTTP_NONE && (flags & KMPGPU_HTTP_HAS_BLANK); o = b.y; l = b.z; break;
    }
    *off = present ? o : 0u;
    *len = present ? l : 0u;
    return present;
}

__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_fields_lengths_kernel(const uint4 *__restrict__ spans, const uint32_t *__restrict__ src_len, uint64_t n, uint32_t field, uint32_t only_present,
                          uint32_t *__restrict__ fld_len, unsigned long long *__restrict__ present, unsigned long long *__restrict__ stats)
{
    const uint32_t lane = threadIdx.x & (KMP_WAVE - 1u), wid = threadIdx.x >> 6;
    const uint64_t n_groups = (n + KMP_WAVE - 1u) / KMP_WAVE;
    GroupSums acc = {0ull, 0ull, 0ull};
    for (uint64_t r = (uint64_t)blockIdx.x * KMP_BLOCK_WAVES + wid; r < n_groups; r += (uint64_t)gridDim.x * KMP_BLOCK_WAVES) {
        const uint64_t k = r * KMP_WAVE + lane;
        const bool in = k < n;
        uint32_t off = 0u, len = 0u;
        bool pres = false;
        if (in) pres = field_of(spans[2u * k], spans[2u * k + 1u], field, &off, &len);
        group_tail(acc, in, k, r, lane, pres, only_present != 0u, in ? src_len[k] : 0u, len, fld_len, present);
    }
    group_sums_flush(acc, lane, stats);
}

/* Payload k of the source is payload j of dst: its slot in the new arena, the field's length, and where the field's bytes lie. */
__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_fields_index_kernel(const uint4 *__restrict__ spans, const uint64_t *__restrict__ src_off, uint32_t field, const uint32_t *__restrict__ fld_len,
                        const uint64_t *__restrict__ loc_off, const uint32_t *__restrict__ loc_idx, const uint64_t *__restrict__ blk_bytes,
                        const uint32_t *__restrict__ blk_cnt, uint64_t n, uint64_t *__restrict__ pkt_off, uint32_t *__restrict__ pkt_len,
                        uint4 *__restrict__ recs)
{
    index_body(fld_len, loc_off, loc_idx, blk_bytes, blk_cnt, n, pkt_off, pkt_len, recs, [&](uint64_t k, uint32_t l) {
        uint32_t off, len;
        field_of(spans[2u * k], spans[2u * k + 1u], field, &off, &len);
        const uint64_t fs = src_off[k] + off;
        return make_uint4((uint32_t)fs, (uint32_t)(fs >> 32), l, 0u);
    });
}

template <bool NT>
__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_fields_gather_kernel(const uint8_t *__restrict__ src, const uint64_t *__restrict__ new_off, const uint4 *__restrict__ recs, uint64_t n,
                         uint64_t total, uint32_t run, uint8_t *__restrict__ dst)
{
    __shared__ uint64_t s_src[KMP_BLOCK_WAVES][KMP_WAVE];          /* where payload i's field starts in src */
    __shared__ uint32_t s_len[KMP_BLOCK_WAVES][KMP_WAVE];
    const uint32_t lane = threadIdx.x & (KMP_WAVE - 1u), wid = threadIdx.x >> 6;
    gather_runs<NT, 2>(new_off, n, total, run, dst,
        [&](uint64_t j, bool in) { return in ? recs[j] : make_uint4(0u, 0u, 0u, 0u); },
        [&](uint4 a) {
            s_src[wid][lane] = ((uint64_t)a.y << 32) | a.x; s_len[wid][lane] = a.z;
        },
        [&](uint32_t p, uint64_t rel64, uint32_t &) {
            const uint32_t F = s_len[wid][p];
            if (rel64 >= (uint64_t)F) return (u32x4)(0u);            /* (an empty payload's slot: zeros) */
            const uint64_t f0 = s_src[wid][p];
            const int32_t fa = (int32_t)(f0 & 15u);                  /* the field in the coordinates of the aligned unit it starts in */
            /* the unit's place in the field, from the aligned unit at or before it so that the offsets stay small */
            const uint64_t ua = (f0 - (uint32_t)fa) + rel64;         /* 16-byte aligned: the first source unit that holds a byte of it */
            const uint64_t left = (uint64_t)F - rel64;
            return fetch_piece<NT>(src + ua, fa, fa, fa + (int32_t)min(left, (uint64_t)16u));
        });
}

}  // namespace

hipError_t kmp_launch_http_locate(const uint8_t *src_arena, const uint64_t *src_off, const uint32_t *src_len, uint64_t n, void *spans,
                                  unsigned long long *stats, hipStream_t st)
{
    static_assert(sizeof(kmpgpu_http_span) == 32, "kmpgpu_http_span is two 16-byte units");
    if (n == 0) return hipSuccess;
    const uint64_t groups = (n + KMP_WAVE - 1) / KMP_WAVE;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((groups + KMP_BLOCK_WAVES - 1) / KMP_BLOCK_WAVES, FLD_LOCATE_BLOCKS);
    hipLaunchKernelGGL(kmp_http_locate_kernel, dim3(blocks), dim3(KMP_BLOCK_THREADS), 0, st, src_arena, src_off, src_len, n,
                       reinterpret_cast<uint4 *>(spans), stats);
    return hipGetLastError();
}

hipError_t kmp_launch_fields_lengths(const void *spans, const uint32_t *src_len, uint64_t n, int field, bool only_present, uint8_t *ws,
                                     unsigned long long *present, unsigned long long *stats, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(kmp_fields_lengths_kernel, dim3(kmp_group_blocks(n)), dim3(KMP_BLOCK_THREADS), 0, st, reinterpret_cast<const uint4 *>(spans), src_len, n,
                       (uint32_t)field, only_present ? 1u : 0u, kmp_compact_ws(ws, n).len, present, stats);
    return hipGetLastError();
}

hipError_t kmp_launch_fields_index(const void *spans, const uint64_t *src_off, uint64_t n, int field, uint8_t *ws, uint64_t n_dst,
                                   uint64_t *pkt_off, uint32_t *pkt_len, void *recs, hipStream_t st)
{
    if (n == 0 || n_dst == 0) return hipSuccess;
    const kmp_compact_view w = kmp_compact_ws(ws, n);
    hipLaunchKernelGGL(kmp_fields_index_kernel, dim3(kmp_item_blocks(n)), dim3(KMP_BLOCK_THREADS), 0, st, reinterpret_cast<const uint4 *>(spans), src_off,
                       (uint32_t)field, w.len, w.loc_off, w.loc_idx, w.blk_bytes, w.blk_cnt, n, pkt_off, pkt_len, reinterpret_cast<uint4 *>(recs));
    return hipGetLastError();
}

hipError_t kmp_launch_fields_gather(const uint8_t *src_arena, const uint64_t *pkt_off, const void *recs, uint64_t n_dst, uint64_t total_bytes,
                                    uint8_t *arena, bool nontemporal, hipStream_t st)
{
    if (n_dst == 0) return hipSuccess;
    const kmp_run_shape rs = kmp_run_shape_of(n_dst, total_bytes);
    hipLaunchKernelGGL(nontemporal ? kmp_fields_gather_kernel<true> : kmp_fields_gather_kernel<false>, dim3(rs.blocks), dim3(KMP_BLOCK_THREADS), 0, st,
                       src_arena, pkt_off, (const uint4 *)recs, n_dst, total_bytes, rs.run, arena);
    return hipGetLastError();
}
