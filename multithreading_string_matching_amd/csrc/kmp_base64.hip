/*
 * kmp_base64.hip -- kmpgpu_load_base64: the base64 runs of an arena's payloads decoded on the device into a packed arena (kmpgpu.h).  gfx950.
 *
 *   kmp_base64_lengths_kernel   dec_len[k] = decoded length of payload k, or 0xFFFFFFFF ("not in dst") for an unchanged payload under
 *                               KMPGPU_B64_ONLY_CHANGED; the changed bitmap, one plain store per word; bytes in / out and n_changed
 *   kmp_scan_local_kernel, kmp_scan_totals_kernel   of kmp_prep.hip, through kmp_launch_compact_scan
 *   kmp_decode_index_kernel     of kmp_decode.hip, through kmp_launch_decode_index: its records {source offset, source length,
 *                               decoded length} are the ones the write here needs
 *   kmp_base64_write_kernel     the bytes
 *
 * The shape is the compacting skeleton's (lengths_body, write_body: kmp_compact_dev.h), as in kmp_decode.hip; what is this
 * file's own is the policy Base64Decode.
 *
 * What a unit cannot decide alone (kmpgpu.h: a run is MAXIMAL, and only a run of min_run bytes and more is decoded):
 *   pre   the length of the alphabet run that ends directly before the unit's first byte, 0 at a payload's first unit.  A unit that is
 *         all alphabet hands on what it got plus 16, any other unit the number of alphabet bytes at its end: a segmented sum, here one
 *         ballot of the "hands on" lanes, a count of the set bits directly below the lane, and one read of the lane that started the
 *         chain.  Lane 0 takes the value the step before left (across the 4-unit unroll as well); pre & 3 is the run offset mod 4.
 *   post  the length of the alphabet run that starts directly behind the unit's last byte, the same chain downwards.  Where the step's
 *         last unit ends inside a run that is still shorter than min_run and its payload goes on, lanes 0..15 load the 16 units behind
 *         it -- whole 16-byte loads, none at or behind the payload's end -- which is all min_run <= 255 can ask for.
 *   pad   how many '=' the unit may drop at its first bytes: 2 or 1 behind a decoded run of m % 4 == 2 or 3 that ends on the unit
 *         before, 1 behind such a run's first '='.  From the lane before, lane 0 from the step before.
 * With these, per unit and in bit arithmetic on 16-bit masks: the decoded runs (head run, tail run, and the inner ones by an erosion
 * and a dilation by min_run), the positions of run offset 0 mod 4 (which yield nothing), and the '=' that are dropped.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kmp_device.h"
#include "kmp_launch.h"
#include "kmp_compact_dev.h"

namespace {

using namespace kmp_unit;     /* kmp_compact_dev.h: lengths_body, write_body; kmp_unit_dev.h: the unit, byte classes */

constexpr uint32_t KMP_B64_LOOKAHEAD = 16;          /* units behind a step that can decide a run: 16 * 16 >= 255 - 1 */

__device__ __forceinline__ uint32_t alpha_bytes(uint32_t w, uint32_t c62, uint32_t c63)
{
    const uint32_t lo7 = w & 0x7F7F7F7Fu;
    const uint32_t dig = (lo7 + 0x50505050u) & ~(lo7 + 0x46464646u);        /* 0x30 <= b <= 0x39 */
    const uint32_t l = lo7 | 0x20202020u;
    const uint32_t let = (l + 0x1F1F1F1Fu) & ~(l + 0x05050505u);            /* 0x61 <= b | 0x20 <= 0x7A */
    return ((dig | let) & ~w & 0x80808080u) | eq_bytes(w, c62) | eq_bytes(w, c63);
}
__device__ __forceinline__ uint32_t alpha16(u32x4 v, uint32_t c62, uint32_t c63)
{
    return bits4(alpha_bytes(v.x, c62, c63)) | bits4(alpha_bytes(v.y, c62, c63)) << 4 | bits4(alpha_bytes(v.z, c62, c63)) << 8 |
           bits4(alpha_bytes(v.w, c62, c63)) << 12;
}
constexpr uint32_t EQ4 = 0x3D3D3D3Du;

/* val() of an alphabet byte: arithmetic, no table.  c62 / c63: the two bytes behind the digits ('+' '/', or '-' '_'), in every byte
 * of the dword as the class tests take them. */
__device__ __forceinline__ uint32_t b64_val(uint32_t b, uint32_t c62, uint32_t c63)
{
    return b == (c63 & 0xFFu) ? 63u : b == (c62 & 0xFFu) ? 62u : b >= 0x61u ? b - 71u : b >= 0x41u ? b - 65u : b + 4u;
}

/* What the step before hands to lane 0: the alphabet run that ends at its last byte, the '=' lane 0 may drop, its last dword. */
struct StepCarry { uint32_t pre, pad, tail_w; };

/* What a unit comes to, the Step of kmp_compact_dev.h: the positions inside the payload, the emitted ones, those inside decoded runs, those
 * of run offset 0 mod 4, the run offset of the byte before the unit (byte() counts it on), the dword before the unit (its last byte is
 * p[i-1] of position 0), and whether the unit holds a byte of a decoded run. */
struct UnitVerdict { uint32_t valid, emit, dec, zero4, r_before, prev_w; bool changed; };

/* Keeps the runs of k and more set bits of x (x: 16 bits; k, p = 4 or 8 the largest of the two <= k, sh = k - p are wave-uniform). */
__device__ __forceinline__ uint32_t runs_of(uint32_t x, uint32_t p, uint32_t sh)
{
    const uint32_t e2 = x & (x >> 1), e4 = e2 & (e2 >> 2), e8 = e4 & (e4 >> 4);
    const uint32_t ep = p == 8u ? e8 : e4;
    const uint32_t ek = ep & (ep >> sh);                        /* bit i: bits i .. i + k - 1 are set */
    const uint32_t d2 = ek | (ek << 1), d4 = d2 | (d2 << 2), d8 = d4 | (d4 << 4);
    const uint32_t dp = p == 8u ? d8 : d4;
    return dp | (dp << sh);
}

__device__ __forceinline__ UnitVerdict step_verdict(const Unit &q, const uint8_t *addr, uint32_t lane, uint32_t min_run, uint32_t c62, uint32_t c63,
                                                    StepCarry &cy)
{
    const uint32_t valid = q.act ? valid_bits(q.len - q.rel) : 0u;
    const uint32_t A = alpha16(q.v, c62, c63) & valid, Q = eq16(q.v, EQ4) & valid;
    const bool firstu = q.rel == 0u, lastu = q.rel + 16u >= q.len, full = A == 0xFFFFu;
    const uint32_t head = (uint32_t)__builtin_ctz(~A);                      /* alphabet bytes at the unit's start, <= 16 */
    const uint32_t tail = (uint32_t)__builtin_clz(~(A << 16));             /* ... at its end */

    /* pre: the lanes directly below that hand on, and the lane (or the step before) that started the chain */
    const uint64_t fwd = __ballot(full && !firstu);
    const uint32_t c_lo = lane ? (uint32_t)__builtin_clzll(~(fwd << (64u - lane)) | 1ull) : 0u;
    const int s_lo = (int)lane - (int)c_lo - 1;
    const uint32_t t_lo = __shfl(tail, s_lo & 63);
    const uint32_t pre = firstu ? 0u : 16u * c_lo + (s_lo >= 0 ? t_lo : cy.pre);
    const uint32_t end_run = full ? pre + 16u : tail;          /* the alphabet run that ends at the unit's last byte */

    /* the run that leaves the step undecided: the 16 units behind the step's last one, as far as its payload has them */
    uint32_t post_step = 0u;
    const bool open_l = q.act && !lastu && end_run != 0u && end_run < min_run;
    if (__builtin_amdgcn_readlane((int)open_l, 63)) {
        const uint32_t rel63 = (uint32_t)__builtin_amdgcn_readlane((int)q.rel, 63), len63 = (uint32_t)__builtin_amdgcn_readlane((int)q.len, 63);
        const uint64_t a63 = bcast64((uint64_t)(uintptr_t)addr, 63u);
        const uint32_t off = rel63 + 16u * (1u + lane);
        uint32_t la = 0u;
        bool la_on = false;
        if (lane < KMP_B64_LOOKAHEAD && off < len63) {
            /* A whole unit as one 16-byte load.  volatile, as the decode's load of the unit behind lane 63: only the alphabet mask of
             * these bytes is used, and without it the compiler may narrow or split the access to the bytes it can prove are needed;
             * payload bytes move in 16-byte loads only.  The units are the ones other lanes hold in the next step's registers; they
             * are read again here so that the steps stay at fixed places and their loads are issued ahead.  off < len63 keeps the
             * load inside the payload's slot: the last unit's slot padding comes with it and is masked off by valid_bits below. */
            const u32x4 w = *(const volatile __attribute__((address_space(1))) u32x4 *)(uintptr_t)(a63 + 16ull * (1u + lane));
            la = alpha16(w, c62, c63) & valid_bits(len63 - off);
            la_on = la == 0xFFFFu && off + 16u < len63;
        }
        const uint32_t n_on = (uint32_t)__builtin_ctzll(~__ballot(la_on));                /* <= 16: lanes 16.. never hand on */
        post_step = 16u * n_on + (uint32_t)__shfl((int)__builtin_ctz(~la), (int)(n_on & 63u));
    }

    /* post: the same chain downwards */
    const uint64_t bwd = __ballot(full && !lastu);
    const uint32_t c_hi = lane < 63u ? (uint32_t)__builtin_ctzll(~(bwd >> (lane + 1u))) : 0u;
    const uint32_t s_hi = lane + c_hi + 1u;
    const uint32_t h_hi = __shfl(head, (int)(s_hi & 63u));
    const uint32_t post = lastu ? 0u : 16u * c_hi + (s_hi < KMP_WAVE ? h_hi : post_step);

    /* decoded runs: the one at the unit's start, the one at its end, the inner ones */
    const uint32_t head_m = (1u << head) - 1u, tail_m = full ? 0u : (0xFFFFu << (16u - tail)) & 0xFFFFu;
    uint32_t D = 0u;
    if (min_run <= 14u) {
        const uint32_t p = min_run >= 8u ? 8u : 4u;
        D = runs_of(A & ~head_m & ~tail_m, p, min_run - p) & 0xFFFFu;
    }
    if (pre + head + (full ? post : 0u) >= min_run) D |= head_m;
    if (tail + post >= min_run) D |= tail_m;

    /* run offset 0 mod 4: the unit's mask behind pre & 3 alphabet bits that stand for the run so far, 20 bits */
    const uint32_t c = pre & 3u;
    const uint32_t X = (A << 4) | (((1u << c) - 1u) << (4u - c));
    const uint32_t p1 = X << 1, p2 = p1 & (p1 << 1), b4 = p2 & (p2 << 2), b8 = b4 & (b4 << 4), b16 = b8 & (b8 << 8);  /* 1..4, ..8, ..16 before */
    uint32_t Z = X & ~p1;                                       /* a run's first byte */
    Z |= (Z << 4) & b4;
    Z |= (Z << 8) & b8;
    Z |= (Z << 16) & b16;
    Z &= X;
    const uint32_t Y1 = (Z << 1) & X, Y2 = (Y1 << 1) & X;       /* run offset 1 and 2 mod 4: m % 4 == 2 and 3 where the run ends there */
    const uint32_t zero4 = (Z >> 4) & 0xFFFFu;
    const uint32_t e2 = D & (Y1 >> 4), e3 = D & (Y2 >> 4);

    /* padding: an '=' directly behind such an end, a second one behind the first of m % 4 == 2 */
    const uint32_t c1a = Q & (e2 << 1), c1b = Q & (e3 << 1), c2 = Q & (c1a << 1);
    const uint32_t pad_out = (e2 >> 15) & 1u ? 2u : ((e3 | c1a) >> 15) & 1u ? 1u : 0u;
    uint32_t pad_in = __shfl_up(pad_out, 1);
    if (lane == 0u) pad_in = cy.pad;
    if (firstu) pad_in = 0u;
    uint32_t cons = c1a | c1b | c2;
    if (pad_in >= 1u && (Q & 1u)) cons |= 1u;
    if (pad_in == 2u && (Q & 3u) == 3u) cons |= 2u;

    uint32_t prev_w = __shfl_up(q.v.w, 1);
    if (lane == 0u) prev_w = cy.tail_w;

    cy.pre = (uint32_t)__builtin_amdgcn_readlane((int)end_run, 63);
    cy.pad = (uint32_t)__builtin_amdgcn_readlane((int)pad_out, 63);
    cy.tail_w = (uint32_t)__builtin_amdgcn_readlane((int)q.v.w, 63);

    UnitVerdict r;
    r.valid = valid;
    r.changed = D != 0u;
    r.dec = D;
    r.zero4 = zero4;
    r.emit = valid & ~(D & zero4) & ~cons & 0xFFFFu;
    r.r_before = (pre - 1u) & 3u;
    r.prev_w = prev_w;
    return r;
}

/* The transform as lengths_body and write_body take it (kmp_compact_dev.h).  Every step needs its neighbours (a run is maximal), so
 * there is no cheap way past step_verdict; a step that decodes nothing and drops no '=' is still stored as it is. */
struct Base64Decode {
    uint32_t min_run, c62, c63;
    StepCarry cy;
    typedef UnitVerdict Step;

    __device__ __forceinline__ void reset() { cy.pre = 0u; cy.pad = 0u; cy.tail_w = 0u; }
    __device__ __forceinline__ Step step(const Unit &q, const uint8_t *addr, uint32_t lane) { return step_verdict(q, addr, lane, min_run, c62, c63, cy); }
    __device__ __forceinline__ uint32_t byte(Step &m, const Unit &q, uint32_t i) const
    {
        const uint32_t ro = (m.zero4 >> i) & 1u ? 0u : (m.r_before + 1u) & 3u;        /* run offset mod 4 of position i */
        m.r_before = ro;
        if (!((m.emit >> i) & 1u)) return 0u;
        const uint32_t w[5] = {m.prev_w, q.v.x, q.v.y, q.v.z, q.v.w};
        const uint32_t b = (w[(i + 4u) >> 2] >> (8u * (i & 3u))) & 0xFFu;
        if (!((m.dec >> i) & 1u)) return b;
        const uint32_t a = (w[(i + 3u) >> 2] >> (8u * ((i + 3u) & 3u))) & 0xFFu;
        return ((b64_val(a, c62, c63) << (2u * ro)) | (b64_val(b, c62, c63) >> (6u - 2u * ro))) & 0xFFu;
    }
};

__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_base64_lengths_kernel(const uint8_t *__restrict__ src, const uint64_t *__restrict__ src_off, const uint32_t *__restrict__ src_len,
                          uint64_t n, uint32_t min_run, uint32_t c62, uint32_t c63, uint32_t only_changed, uint32_t *__restrict__ dec_len,
                          unsigned long long *__restrict__ changed, unsigned long long *__restrict__ stats)
{
    lengths_body(src, src_off, src_len, n, only_changed, dec_len, changed, stats, Base64Decode{min_run, c62, c63, {0u, 0u, 0u}});
}

template <bool NT>
__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
kmp_base64_write_kernel(const uint8_t *__restrict__ src, const uint64_t *__restrict__ new_off, const uint4 *__restrict__ recs, uint64_t n,
                        uint64_t total, uint32_t run, uint32_t min_run, uint32_t c62, uint32_t c63, uint8_t *__restrict__ dst)
{
    write_body<NT>(src, new_off, recs, n, total, run, dst, Base64Decode{min_run, c62, c63, {0u, 0u, 0u}});
}

}  // namespace

/* Phase 1: decoded lengths, changed bitmap, stats.  ws, changed, stats: as kmp_launch_decode_lengths. */
hipError_t kmp_launch_base64_lengths(const uint8_t *src_arena, const uint64_t *src_off, const uint32_t *src_len, uint64_t n, uint32_t min_run,
                                     bool urlsafe, bool only_changed, uint8_t *ws, unsigned long long *changed, unsigned long long *stats,
                                     hipStream_t st)
{
    if (n == 0) return hipSuccess;
    const uint32_t c62 = urlsafe ? 0x2D2D2D2Du : 0x2B2B2B2Bu, c63 = urlsafe ? 0x5F5F5F5Fu : 0x2F2F2F2Fu;
    hipLaunchKernelGGL(kmp_base64_lengths_kernel, dim3(kmp_group_blocks(n)), dim3(KMP_BLOCK_THREADS), 0, st, src_arena, src_off, src_len, n, min_run,
                       c62, c63, only_changed ? 1u : 0u, kmp_compact_ws(ws, n).len, changed, stats);
    return hipGetLastError();
}

hipError_t kmp_launch_base64_write(const uint8_t *src_arena, const uint64_t *pkt_off, const void *recs, uint64_t n_dst, uint64_t bytes_in,
                                   uint64_t total_bytes, uint32_t min_run, bool urlsafe, uint8_t *arena, bool nontemporal, hipStream_t st)
{
    if (n_dst == 0) return hipSuccess;
    const kmp_run_shape rs = kmp_run_shape_of(n_dst, bytes_in > total_bytes ? bytes_in : total_bytes);       /* a run's SOURCE bytes count as well */
    const uint32_t c62 = urlsafe ? 0x2D2D2D2Du : 0x2B2B2B2Bu, c63 = urlsafe ? 0x5F5F5F5Fu : 0x2F2F2F2Fu;
    hipLaunchKernelGGL(nontemporal ? kmp_base64_write_kernel<true> : kmp_base64_write_kernel<false>, dim3(rs.blocks), dim3(KMP_BLOCK_THREADS), 0, st,
                       src_arena, pkt_off, (const uint4 *)recs, n_dst, total_bytes, rs.run, min_run, c62, c63, arena);
    return hipGetLastError();
}
