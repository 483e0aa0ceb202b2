/*
 * kmp_scan_stream_kernels.inc -- the two streaming kernels of kmp_scan_stream.hip, which includes this text twice inside its
 * anonymous namespace:
 *   KMP_WHOLE false, KMP_FLAT_KERNEL = kmp_scan_flat_kernel, KMP_PACKED_KERNEL = kmp_scan_packed_kernel: the reference's rule,
 *       a payload is text up to its first 0x00 (the default);
 *   KMP_WHOLE true, kmp_scan_flat_whole_kernel / kmp_scan_packed_whole_kernel: KMPGPU_OPT_WHOLE_PAYLOAD, text up to the payload's end.
 * Two compilations of one text rather than a template parameter or a shared __device__ body: the default kernels keep their names
 * (tests/test_isa.py selects them by name) and their code, instruction for instruction.
 */
/* ================================================================================================
 * Uniform-stride arenas (every payload the same length, slots back to back): flat streaming.
 *
 * Each wavefront owns a CONTIGUOUS run of packets, i.e. one contiguous byte range of the arena,
 * and streams it in 1 KiB chunks irrespective of packet boundaries: every lane always holds 16
 * useful bytes, consecutive chunk loads are consecutive addresses, and there is no per-packet
 * scalar work at all.  Because slots are 16-byte aligned a lane's 16 bytes belong to exactly one
 * packet; the lane tracks p0 = offset of its first byte inside that packet's slot with one
 * add + min per chunk.  Still one packet per wavefront at a time: the packets of a range are
 * scanned in order by the same wavefront, so the "first 0x00 ends the text" rule (serial.c:191)
 * is wave-local state (dead: the packet entering the chunk already had a NUL).
 *
 * A start offset s (lane position i, s = p0 + i) counts iff
 *     s + m <= L                       window inside the payload                  (serial.c:193,198)
 *     no 0x00 in the packet before s   strlen() stopped earlier otherwise         (serial.c:191)
 *     text[s : s+m] == pattern         (a NUL inside the window fails here: patterns are NUL-free)
 * ============================================================================================== */


/* KMP_WHOLE (KMPGPU_OPT_WHOLE_PAYLOAD): the text of a payload is all of it, E = L.  The 0x00 test, its ballot, the `dead` carry and
 * nul_limit are not compiled in; a 0x00 is a text byte like any other, which no pattern holds.  What is left of the rule is the
 * payload's end: maxi = L - m - p0. */
template <int DEPTH, bool NT, bool EMIT = false>
__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
KMP_FLAT_KERNEL(const uint8_t *__restrict__ arena, uint64_t n_pkts, uint32_t stride, uint32_t L,
                uint32_t pkts_per_wave, const kmp_pattern_dev *__restrict__ patterns,
                const uint32_t *__restrict__ pat_ids, unsigned long long *__restrict__ partials, unsigned long long *__restrict__ zero_counts, Emitter em)
{
    __shared__ unsigned long long s_wave_cnt[KMP_BLOCK_WAVES];

    const uint32_t lane = threadIdx.x & (KMP_WAVE - 1u);
    const uint32_t wave = sgpr(threadIdx.x >> 6);
    const uint64_t gw = (uint64_t)blockIdx.x * KMP_BLOCK_WAVES + wave;
    /* this wavefront's packets [k0, k1) = bytes [0, range) behind base */
    const uint64_t k0 = gw * pkts_per_wave;
    const uint64_t k1 = min(n_pkts, k0 + pkts_per_wave);
    const uint32_t range = (k0 < n_pkts) ? (uint32_t)(k1 - k0) * stride : 0u;      /* host guarantees < 2^31 */
    const uint8_t *base = arena + ((k0 < n_pkts) ? k0 * (uint64_t)stride : 0ull);
    const uint32_t step_mod = KMP_CHUNK % stride;                                    /* p0 advance per chunk (mod stride) */

    /* The stream starts before anything else: the first DEPTH chunk loads need nothing but the range, and the
     * 2 us they take cover the fetch of the pattern record below (an empty range has a record count of 0: its
     * loads fetch nothing and return zeros). */
    const i32x4    rsrc = make_rsrc(base, range);
    const uint32_t vo0 = lane * KMP_LANE_BYTES;
    u32x4 buf[DEPTH];
#pragma unroll
    for (int s = 0; s < DEPTH; ++s) flat_issue<NT, true>(buf[s], rsrc, vo0, (uint32_t)s * KMP_CHUNK);

    const uint32_t pid = pat_ids[blockIdx.y];
    const kmp_pattern_dev *gp = patterns + pid;
    const PatConst pc = load_pat_const(gp);
    const uint32_t m = pc.m;
    if (EMIT) em.pattern = pid;
    if (EMIT && em.windows) {                /* this block's window, once: pid is uniform, a scalar load */
        const uint2 win = em.windows[pid];
        em.win_first = win.x; em.win_last = win.y;
    }

    uint32_t cnt = 0u;
    {
        uint32_t p0 = vo0 % stride;          /* offset of this lane's first byte inside its packet's slot */
        bool     dead = false;               /* the packet that enters the chunk already had a 0x00      */
        uint32_t cb = 0u;                    /* byte offset of the chunk being consumed                   */

        while (cb < range) {
#pragma unroll
            for (int s = 0; s < DEPTH; ++s) {
                ring_wait<DEPTH - 2>(buf[s], buf[(s + 1) % DEPTH]);
                if (cb < range) {
                    const uint4    v   = make_uint4(buf[s].x, buf[s].y, buf[s].z, buf[s].w);
                    const u32x4    bn  = buf[(s + 1) % DEPTH];                /* next chunk (zeros past the range) */
                    const uint32_t w[5] = {v.x, v.y, v.z, v.w, wave_shl1(v.x, sgpr(bn.x))};

                    uint64_t S[4];
                    uint32_t t[4];
                    if constexpr (KMP_WHOLE) {
                        const uint32_t fz = zero_half_mask(filter_sad(w, pc.p[0], S, t));
                        if (ballot64(fz != 0u) != 0ull) {
                            /* rare path: the payload's end is all that bars a start offset */
                            int32_t maxi = (int32_t)L - (int32_t)m - (int32_t)p0;
                            if (fz == 0u) maxi = -1;
                            const uint64_t pkt = EMIT ? (k0 + (uint64_t)((cb + vo0 - p0) / stride)) : 0ull;
                            confirm_sad<EMIT>(S, t, w, v, bn, fz, maxi, p0, pc, gp, cnt, pkt, em);
                        }
                    } else {
                    const uint32_t zm = zero_byte_mask(w[0]) | zero_byte_mask(w[1]) | zero_byte_mask(w[2]) | zero_byte_mask(w[3]);
                    const uint32_t fz = zero_half_mask(filter_sad(w, pc.p[0], S, t));      /* != 0 iff the lane has a candidate */
                    const uint64_t zl = ballot64(zm != 0u);                   /* lanes holding a 0x00           */
                    const uint64_t st = ballot64(p0 == 0u);                   /* lanes where a packet starts    */
                    const uint64_t cl = ballot64(fz != 0u);                   /* lanes with a candidate         */
                    const bool dead_in = dead;
                    /* carry for the next chunk: is there a 0x00 at or after the last packet start of this chunk? */
                    if (zl == 0ull) { if (st != 0ull) dead = false; }
                    else            dead = (st == 0ull) ? true : ((zl >> (63u - (uint32_t)__builtin_clzll(st))) != 0ull);

                    if (cl != 0ull) {
                        /* rare path.  maxi = largest start index (0..15) of this lane that still counts:
                         * window inside the payload, no 0x00 before it, lane has a candidate at all. */
                        int32_t maxi = (int32_t)L - (int32_t)m - (int32_t)p0;
                        if (fz == 0u) maxi = -1;
                        if (zl != 0ull || dead_in) {
                            /* A 0x00 in the LAST lane of a packet (slot padding, a trailer) ends nothing but that lane's own
                             * later offsets -- and matters only if that lane has a candidate; the segmented form is for a
                             * 0x00 in mid-packet. */
                            const uint64_t last_lanes = ballot64(p0 + KMP_LANE_BYTES == stride);
                            if (dead_in || (zl & ~last_lanes) != 0ull) maxi = nul_limit(maxi, w, zl, st, dead_in, lane);
                            else if (ballot64(zm != 0u && fz != 0u) != 0ull) maxi = nul_limit(maxi, w, 0ull, st, false, lane);
                        }
                        const uint64_t pkt = EMIT ? (k0 + (uint64_t)((cb + vo0 - p0) / stride)) : 0ull;
                        confirm_sad<EMIT>(S, t, w, v, bn, fz, maxi, p0, pc, gp, cnt, pkt, em);
                    }
                    }
                    /* this lane's position inside its packet, one chunk further */
                    p0 += step_mod;
                    p0 = min(p0, p0 - stride);               /* unsigned: subtracts stride iff p0 >= stride */
                }
                __builtin_amdgcn_sched_barrier(0);
                flat_issue<NT>(buf[s], rsrc, vo0, cb + (uint32_t)DEPTH * KMP_CHUNK);
                cb += KMP_CHUNK;
            }
        }
#pragma unroll
        for (int s = 0; s < DEPTH; s += 2) ring_wait<0>(buf[s], buf[(s + 1) % DEPTH]);
    }

    unsigned long long c64 = cnt;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c64 += __shfl_xor(c64, o);
    if (lane == 0u) s_wave_cnt[wave] = c64;
    __syncthreads();
    if (threadIdx.x == 0u) {
        unsigned long long t = 0ull;
#pragma unroll
        for (uint32_t i = 0; i < KMP_BLOCK_WAVES; ++i) t += s_wave_cnt[i];
        partials[(uint64_t)blockIdx.y * gridDim.x + blockIdx.x] = t;
        /* a launch of tens of thousands of blocks is summed by several blocks of kmp_reduce_kernel, each of which ADDS its share
         * to the pattern's counter: unless the pass accumulates, the counter starts from 0 here, a kernel boundary ahead of them */
        if (zero_counts && blockIdx.x == 0u) zero_counts[pid] = 0ull;
    }
}

/* KMP_WHOLE: as in the flat kernel.  The payload's end comes from the start bitmap (clean padding) or from the index, as in the default
 * pass -- where a 0x00 usually ended the text first. */
template <int DEPTH, bool NT, bool EMIT = false>
__global__ void __launch_bounds__(KMP_BLOCK_THREADS)
KMP_PACKED_KERNEL(const uint8_t *__restrict__ arena, const uint64_t *__restrict__ pkt_off,
                  const uint32_t *__restrict__ pkt_len, const unsigned long long *__restrict__ bitmap,
                  const kmp_plan_entry *__restrict__ plan, const kmp_pattern_dev *__restrict__ patterns,
                  const uint32_t *__restrict__ pat_ids, unsigned long long *__restrict__ partials, unsigned long long *__restrict__ zero_counts, Emitter em,
                  uint32_t pad_clean)
{
    __shared__ unsigned long long s_wave_cnt[KMP_BLOCK_WAVES];

    const uint32_t lane = threadIdx.x & (KMP_WAVE - 1u);
    const uint32_t wave = sgpr(threadIdx.x >> 6);
    const uint64_t gw = (uint64_t)blockIdx.x * KMP_BLOCK_WAVES + wave;
    const uint64_t k0 = plan[gw].k, k1 = plan[gw + 1].k;
    /* The range starts at a packet start (16-byte aligned).  Streaming from there would make every 1 KiB chunk
     * load straddle nine 128-byte lines instead of covering eight, and the line shared by two consecutive
     * chunks is fetched from HBM twice under the streaming (nt) policy: +4.5 % traffic measured.  So the
     * stream starts on the line boundary below; the `pl` lanes of the first chunk that precede the first
     * packet belong to the previous wavefront and are blanked (zero bytes, no start bits). */
    const uint64_t off_first = plan[gw].off;
    const uint32_t pre = (uint32_t)(off_first & 127ull), pl = pre >> 4;
    const uint64_t off0 = off_first - pre;
    const uint32_t range = (k1 > k0) ? (uint32_t)(plan[gw + 1].off - off0) : 0u;    /* planner guarantees < 2^31 */

    /* the stream starts before the pattern record is staged (see kmp_scan_flat_kernel); an empty range fetches nothing */
    const i32x4    rsrc = make_rsrc(arena + off0, range);
    const uint32_t vo0 = lane * KMP_LANE_BYTES;
    u32x4 buf[DEPTH];
#pragma unroll
    for (int s = 0; s < DEPTH; ++s) flat_issue<NT, true>(buf[s], rsrc, vo0, (uint32_t)s * KMP_CHUNK);

    const uint32_t pid = pat_ids[blockIdx.y];
    const kmp_pattern_dev *gp = patterns + pid;
    const PatConst pc = load_pat_const(gp);
    const uint32_t m = pc.m;
    if (EMIT) em.pattern = pid;
    if (EMIT && em.windows) {                /* this block's window, once: pid is uniform, a scalar load */
        const uint2 win = em.windows[pid];
        em.win_first = win.x; em.win_last = win.y;
    }

    uint32_t cnt = 0u;
    if (range) {
        /* packet-start bits of chunk j: bits [b0 + 64 j, +64) of the bitmap = words wi0+j, wi0+j+1 shifted by sh */
        const uint64_t b0 = off0 >> 4;
        const unsigned long long *bw = bitmap + (b0 >> 6);
        const uint32_t sh = (uint32_t)(b0 & 63ull);

        unsigned long long hiw[DEPTH];       /* bitmap word wi0 + j + 1 of the chunk in ring slot s, fetched one group ahead */
#pragma unroll
        for (int s = 0; s < DEPTH; ++s) hiw[s] = bw[s + 1];
        unsigned long long low = bw[0];      /* bitmap word wi0 + j of the chunk being consumed */
        uint64_t kbase = k0 - 1ull;          /* index of the last packet started before the chunk */
        bool     dead = false;
        uint32_t cb = 0u, j = 0u;

        while (cb < range) {
            /* Packet-start words, one GROUP of ring slots ahead.  Scalar loads return out of order, so the only
             * wait that covers them is lgkmcnt(0) -- which also waits for a load issued a moment ago.  Using this
             * group's words first (they have had a whole group of chunks to arrive) and only then asking for the
             * next group's keeps that wait off the critical path. */
            uint64_t st_[DEPTH];
#pragma unroll
            for (int s = 0; s < DEPTH; ++s) {
                const unsigned long long hi = hiw[s];
                st_[s] = sh ? ((low >> sh) | (hi << (64u - sh))) : low;                   /* lanes where a packet starts */
                low = hi;
                asm volatile("" : "+s"(st_[s]));      /* computed HERE, not sunk below the loads that follow */
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int s = 0; s < DEPTH; ++s) hiw[s] = bw[j + (uint32_t)DEPTH + 1u + (uint32_t)s];
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int s = 0; s < DEPTH; ++s) {
                ring_wait<DEPTH - 2>(buf[s], buf[(s + 1) % DEPTH]);
                if (cb < range) {
                    uint4          v   = make_uint4(buf[s].x, buf[s].y, buf[s].z, buf[s].w);
                    const u32x4    bn  = buf[(s + 1) % DEPTH];
                    uint64_t       st  = st_[s];
                    if (s == 0 && cb == 0u && pl != 0u) {                               /* head of the range, see above */
                        if (lane < pl) v = make_uint4(0u, 0u, 0u, 0u);
                        st &= ~0ull << pl;
                    }
                    const uint32_t w[5] = {v.x, v.y, v.z, v.w, wave_shl1(v.x, sgpr(bn.x))};

                    uint32_t zm = 0u;
                    if constexpr (!KMP_WHOLE) zm = zero_byte_mask(w[0]) | zero_byte_mask(w[1]) | zero_byte_mask(w[2]) | zero_byte_mask(w[3]);
                    uint64_t S[4];
                    uint32_t t[4];
                    const uint32_t fz = zero_half_mask(filter_sad(w, pc.p[0], S, t));      /* != 0 iff the lane has a candidate */
                    uint64_t zl = 0ull;
                    if constexpr (!KMP_WHOLE) zl = ballot64(zm != 0u);
                    const uint64_t cl = ballot64(fz != 0u);
                    const bool dead_in = dead;
                    if constexpr (!KMP_WHOLE) {
                    if (zl == 0ull) { if (st != 0ull) dead = false; }
                    else            dead = (st == 0ull) ? true : ((zl >> (63u - (uint32_t)__builtin_clzll(st))) != 0ull);
                    }

                    if (cl != 0ull) {
                        /* rare path: which packet does a candidate lane sit in? */
                        int32_t  maxi = -1;
                        uint32_t p0 = 0u, L = 0u;
                        uint64_t kl = 0ull;
                        uint64_t nx;                                                    /* start bits of the next chunk */
                        if (s + 1 < DEPTH) nx = st_[(s + 1) % DEPTH];
                        else               nx = sh ? ((low >> sh) | (hiw[0] << (64u - sh))) : low;
                        const uint64_t last_lanes = (st >> 1) | (nx << 63);           /* the lanes behind which a packet starts */
                        if (!EMIT && pad_clean && m <= 16u && (cl & last_lanes) == 0ull) {
                            /* (see the next branch) no candidate sits in the last lane of its slot: every one of them has 32
                             * bytes of slot or more from its first byte, all 16 start offsets fit a pattern of up to 16 bytes */
                            maxi = fz != 0u ? 15 : -1;
                        } else if (!EMIT && pad_clean) {
                            /* Slot padding is all 0x00 (checked when the arena was loaded), so "the window lies inside
                             * the payload" = "it lies inside the slot and holds no 0x00": the distance to the next
                             * packet start, read off the bitmap, replaces the payload's offset and length -- no
                             * gather from the index, which costs a memory round trip per candidate chunk. */
                            if (fz != 0u) {
                                const uint64_t above = (st >> 1) >> lane;               /* starts at the lanes above own */
                                uint32_t d = 4096u;                                     /* 16-byte groups up to the next start */
                                if (above != 0ull) d = (uint32_t)__builtin_ctzll(above) + 1u;
                                else if (nx != 0ull) d = 64u - lane + (uint32_t)__builtin_ctzll(nx);
                                L = d * KMP_LANE_BYTES;                                 /* bytes from the lane's first to the slot's end */
                                maxi = (int32_t)L - (int32_t)m;
                            }
                        } else if (fz != 0u) {
                            const uint64_t le = (2ull << lane) - 1ull;                  /* lanes <= own (lane 63: all ones) */
                            kl = kbase + (uint64_t)__builtin_popcountll(st & le);
                            const uint64_t po = pkt_off[kl];
                            L  = pkt_len[kl];
                            p0 = (uint32_t)(off0 + cb + vo0 - po);
                            maxi = (int32_t)L - (int32_t)m - (int32_t)p0;
                        }
                        if constexpr (!KMP_WHOLE) {
                        if (zl != 0ull || dead_in) {
                            /* a 0x00 in the last lane of a packet ends nothing but that lane's own later offsets (see kmp_scan_flat_kernel) */
                            if (dead_in || (zl & ~last_lanes) != 0ull) maxi = nul_limit(maxi, w, zl, st, dead_in, lane);
                            else if (ballot64(zm != 0u && fz != 0u) != 0ull) maxi = nul_limit(maxi, w, 0ull, st, false, lane);
                        }
                        }
                        confirm_sad<EMIT>(S, t, w, v, bn, fz, maxi, p0, pc, gp, cnt, kl, em);
                        /* leave nothing of the rare path's LDS/scalar reads "possibly in flight": merged into the
                         * common path that state costs an s_waitcnt lgkmcnt(0) per chunk, which would also wait
                         * for the bitmap words just asked for */
                        __builtin_amdgcn_s_waitcnt(0xC07F);      /* lgkmcnt(0) only */
                    }
                    kbase += (uint64_t)__builtin_popcountll(st);
                }
                __builtin_amdgcn_sched_barrier(0);
                flat_issue<NT>(buf[s], rsrc, vo0, cb + (uint32_t)DEPTH * KMP_CHUNK);
                cb += KMP_CHUNK;
                ++j;
            }
        }
    }
#pragma unroll
    for (int s = 0; s < DEPTH; s += 2) ring_wait<0>(buf[s], buf[(s + 1) % DEPTH]);     /* nothing in flight when the wavefront ends */

    unsigned long long c64 = cnt;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c64 += __shfl_xor(c64, o);
    if (lane == 0u) s_wave_cnt[wave] = c64;
    __syncthreads();
    if (threadIdx.x == 0u) {
        unsigned long long t = 0ull;
#pragma unroll
        for (uint32_t i = 0; i < KMP_BLOCK_WAVES; ++i) t += s_wave_cnt[i];
        partials[(uint64_t)blockIdx.y * gridDim.x + blockIdx.x] = t;
        /* a launch of tens of thousands of blocks is summed by several blocks of kmp_reduce_kernel, each of which ADDS its share
         * to the pattern's counter: unless the pass accumulates, the counter starts from 0 here, a kernel boundary ahead of them */
        if (zero_counts && blockIdx.x == 0u) zero_counts[pid] = 0ull;
    }
}

