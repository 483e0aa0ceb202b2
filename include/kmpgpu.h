/*
 * kmpgpu.h -- C-ABI of the MI355X (gfx950) KMP match-count hot path.
 *
 * The reference has no FFI: its hot path is the loop
 *     string_count[i] += kmp_matcher(array_of_payloads[k], array_of_strings[i], prefix_array[i]);
 * at serial.c:153-155 (= openmp_data.c:157-175, mpi_dumping.c:198-200) with kmp_matcher at
 * serial.c:190-215 and kmp_prefix at serial.c:217-238.  A maintainer replaces that loop by the
 * calls below (INTEGRATION.md shows the patch).  Library:
 * multithreading_string_matching_amd/lib/libkmpgpu.so (hipcc, --offload-arch=gfx950).
 *
 * Semantics: payload k of length L_k is text up to E_k, and count[i] = sum over k of the number of start offsets s with
 * s + m_i <= E_k and payload_k[s : s+m_i] == pattern_i (overlapping starts all count; a window never leaves its payload).
 *   E_k = min(L_k, index of its first 0x00)   the reference's rule (kmp_matcher takes strlen() of the payload, serial.c:191;
 *                                             SURVEY.md App. A), bit-exact with compiled serial.c.  The default.
 *   E_k = L_k                                 whole payloads, KMPGPU_OPT_WHOLE_PAYLOAD = 1: a 0x00 is a text byte like any other
 *                                             (which matches nothing: patterns hold none).  Not the reference's behaviour.
 * Everything that counts, reports or marks matches -- kmpgpu_scan, kmpgpu_scan_enqueue, kmpgpu_scan_offsets,
 * kmpgpu_scan_packets, kmpgpu_scan_rules, kmpgpu_scan_relations, kmpgpu_scan_chains, with or without KMPGPU_PAT_NOCASE -- uses the E_k of the option's value at the time of the call.
 *
 * Conventions: plain pointers and sizes only; every function returns 0 or a negative KMPGPU_E*
 * code and never exits; kmpgpu_last_error() gives the text (per thread).  One context drives one GPU;
 * several GPUs = several contexts, in one process or one process each, whose counters are summed by
 * RCCL (kmpgpu_comm_*, the MPI_Reduce of mpi_dumping.c:202).  A context is not thread-safe; different
 * contexts may be driven from different threads.  Host buffers passed in are borrowed for the call; device buffers created
 * by the context are owned by it.
 */
#ifndef KMPGPU_H
#define KMPGPU_H

#include <stddef.h>
#include <stdint.h>

#include "kmp_synth.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KMPGPU_OK         0
#define KMPGPU_EHIP      -1   /* a HIP runtime call failed (no device, out of memory ...)  */
#define KMPGPU_EINVAL    -2   /* bad argument / layout contract violated                    */
#define KMPGPU_ESTATE    -3   /* call order: patterns or arena not set                      */
#define KMPGPU_ENOMEM    -4

#define KMPGPU_MAX_PATTERN_LEN 99      /* serial.c:64 */
#define KMPGPU_SLOT_ALIGN      16

typedef struct kmpgpu_ctx kmpgpu_ctx;

/* Timing of the last kmpgpu_scan / kmpgpu_load_arena on this context (HIP events on the
 * context's stream). */
typedef struct kmpgpu_timing {
    double   h2d_ms;          /* arena + index upload (kmpgpu_load_arena)                  */
    double   kernel_ms;       /* scan kernel(s) + partial-count reduce                     */
    double   d2h_ms;          /* counts download                                           */
    uint32_t launches;        /* scan-kernel launches in the last scan                     */
    uint32_t grid_blocks;     /* blocks per launch (x dimension)                           */
    uint64_t h2d_bytes;       /* bytes the last kmpgpu_load_arena / kmpgpu_load_frames copied to the device */
} kmpgpu_timing;

/* One reported match (kmpgpu_scan_offsets).  Not in the reference, which prints counts only
 * (serial.c:163-166); BASELINE north_star asks for offsets. */
typedef struct kmpgpu_match {
    uint64_t packet;          /* payload index in the arena                                */
    uint32_t offset;          /* start offset inside the payload                           */
    uint32_t pattern;         /* pattern index (file order)                                */
} kmpgpu_match;

/* Option keys for kmpgpu_set_option. */
#define KMPGPU_OPT_MODE          1   /* 0 auto (filter + KMP verify), 1 KMP automaton only */
#define KMPGPU_OPT_BLOCKS_PER_CU 2   /* grid = CUs * this (1..256); 0 = auto (default): the streaming kernels
                                        take ~6-16 KiB per wavefront, however many blocks that is */
#define KMPGPU_OPT_DEPTH         3   /* chunk loads in flight per wavefront: 2..6, 8; 0 = auto */
#define KMPGPU_OPT_FUSED         4   /* 1 = fused multi-pattern pass: the patterns of 2..99
                                        bytes are counted in ONE read of a packed arena per 1024
                                        distinct patterns (256 where 2-byte patterns are among
                                        them; up to four 1-byte patterns ride along,
                                        further ones keep one read each); 0 = off; 2 = auto
                                        (default): fused from 2 such unique patterns on         */
#define KMPGPU_OPT_KERNEL        5   /* 0 auto: slots back to back -> packed streaming kernel, or
                                        the flat streaming kernel when every payload has the same
                                        length of 512 bytes or more (also taken for equal slots
                                        with gaps between them); otherwise the general kernel.
                                        1 always the general one-packet-per-wavefront kernel;
                                        2 the packed kernel whenever the slots are back to back;
                                        3 the flat kernel whenever the stride is uniform          */

#define KMPGPU_OPT_ACCUMULATE    6   /* 1 = every pass ADDS to the counts buffer instead of
                                        overwriting it (batches of a streamed capture,
                                        openmp_task.c:172-175); kmpgpu_counts_reset() zeroes it */

#define KMPGPU_OPT_REPACK        7   /* 1 (default) = an arena whose slots are not back to back is
                                        copied once, on the device, into a packed arena owned by
                                        the context (streaming kernels); 0 = scan it in place
                                        with the general kernel                                 */
#define KMPGPU_OPT_FUSED_UNIT    8   /* fused pass: bytes of a work unit of the pool at the end of a region (a multiple
                                        of 1024 up to 1 MiB; 0 = auto, 32 KiB; larger where a region has more than ~220 of
                                        them): a wavefront that is through its own share of the region takes the pool's
                                        units one after the other */
#define KMPGPU_OPT_WHOLE_PAYLOAD 9   /* 0 (default) = a payload is text up to its first 0x00, the reference's strlen() rule; 1 = up to
                                        its end (E_k = L_k, "Semantics" above); any other value: KMPGPU_EINVAL.  Pass state, not
                                        arena or pattern state: it holds from the next pass on, for every way a pass is made, and may
                                        be switched between two scans of one context with nothing reloaded, re-attached or re-set.
                                        Patterns stay free of 0x00 either way.  The whole-payload kernels keep 4 chunk loads in
                                        flight (the fused pass 3, as always): KMPGPU_OPT_DEPTH is accepted and has no effect on them */
#define KMPGPU_OPT_KEEP_META    10   /* 0 (default) = kmpgpu_load_frames / _begin builds the arena alone, exactly as without this option;
                                        1 = one further kernel keeps the per-payload header metadata of every accepted frame
                                        (kmpgpu_pkt_meta, below); any other value: KMPGPU_EINVAL.  Read when a load is begun */
#define KMPGPU_OPT_FLOW_SLOTS   11   /* slots of the hash table kmpgpu_flows_build groups the payloads in: 0 (default) = auto, the smallest
                                        power of two >= 2 x n_pkts; any other value must be a power of two > n_pkts, or kmpgpu_flows_build
                                        returns KMPGPU_EINVAL (negative: kmpgpu_set_option does).  A tuning knob like KMPGPU_OPT_DEPTH: no
                                        output depends on it */
#define KMPGPU_OPT_NONTEMPORAL 100   /* 1 (default) = arena loads carry the non-temporal hint (every
                                        byte is read once per pass; measured +10 % on MI355X), 0 =
                                        default cache policy                                   */

const char *kmpgpu_last_error(void);
int  kmpgpu_device_count(void);                        /* >= 0, or KMPGPU_EHIP                */

/* Create / destroy the context for one device.  Replaces nothing in the reference (its state
 * lives in main()'s locals, serial.c:99-101,148). */
int  kmpgpu_init(kmpgpu_ctx **ctx, int device);
void kmpgpu_destroy(kmpgpu_ctx *ctx);

/* Launch on a caller-owned HIP stream (hipStream_t, e.g. an explicit torch stream); NULL returns
 * to the context's own (non-blocking) stream.  The legacy default stream has the handle NULL and
 * therefore cannot be borrowed: create an explicit stream when work must be ordered with the
 * caller's (bench.py does). */
int  kmpgpu_set_stream(kmpgpu_ctx *ctx, void *hip_stream);
int  kmpgpu_set_option(kmpgpu_ctx *ctx, int key, int64_t value);

/* Pinned host memory for the arena (north_star: "pinned contiguous arena"). */
void *kmpgpu_host_alloc(size_t bytes);
void  kmpgpu_host_free(void *p);
/* Pin memory the caller already has -- e.g. (a window of) a capture file's read-only mapping -- so that uploads from it
 * (kmpgpu_load_frames, kmpgpu_load_arena) run as asynchronous DMA at PCIe speed instead of being staged through the runtime's
 * bounce buffers.  ptr page-aligned.  Returns KMPGPU_EHIP where the runtime refuses (then the memory simply stays pageable). */
int   kmpgpu_host_register(const void *ptr, size_t bytes);
int   kmpgpu_host_unregister(const void *ptr);

/* Replaces array_of_strings + prefix_array construction, serial.c:148-152 (kmp_prefix for every
 * pattern): copies the patterns, builds the failure tables on the host, uploads both.
 * 1 <= pat_len[i] <= 99, no 0x00 inside a pattern (fscanf("%s") + strlen cannot produce one). */
int  kmpgpu_set_patterns(kmpgpu_ctx *ctx, const uint8_t *const *pat, const uint32_t *pat_len, uint32_t n_pat);

/* Case-insensitive patterns (not in the reference; grep -i, Snort / Suricata "nocase").  flags[i] (NULL = all 0) carries
 * KMPGPU_PAT_NOCASE for pattern i; every other bit is reserved and rejected with KMPGPU_EINVAL.  kmpgpu_set_patterns(...) is
 * kmpgpu_set_patterns_flags(..., NULL, ...).  For a nocase pattern ASCII letters match either case (0x41..0x5A equal
 * 0x61..0x7A); every other byte compares exactly (0x40 '@', 0x5B '[', 0x60 '`', 0x7B '{' and all of 0x80..0xFF: 0xC1 is not
 * 0xE1); E_k (which follows KMPGPU_OPT_WHOLE_PAYLOAD), overlapping starts, 1..99 bytes and no 0x00 are as above.  Formally
 *     count_nocase(payloads, p) == count(fold(payloads), fold(p)),  fold = lowercase ASCII A-Z only,
 * and kmpgpu_scan_offsets reports the (packet, offset, pattern) of that formulation, pattern = the caller's index.  Flags are
 * per pattern: one set may mix both kinds, and the same bytes may appear with both flags, each index counted on its own.
 * Cost: the nocase patterns that hold an ASCII letter are counted over a folded copy of the arena that the context owns
 * (same layout; the caller's arena is never written, kmpgpu_arena_download returns the original bytes), made once per
 * arena -- on the context's stream at the start of the first pass after a load / attach / repack, inside kernel_ms, not a
 * launch of kmpgpu_timing -- and grown like the other device buffers (kmpgpu_reserve sizes it when the patterns need it).
 * All-nocase set: that fold (one read + one write of the arena), then exactly the passes of the folded set taken
 * case-sensitively.  Mixed set: the fold, the case-sensitive passes and the nocase passes -- at least two reads of the
 * arena per scan.  A nocase pattern without a letter is its case-sensitive self and costs nothing extra. */
#define KMPGPU_PAT_NOCASE 1u
int  kmpgpu_set_patterns_flags(kmpgpu_ctx *ctx, const uint8_t *const *pat, const uint32_t *pat_len,
                               const uint32_t *flags /* NULL = all 0 */, uint32_t n_pat);

/* Replaces array_of_payloads, serial.c:99,124-136: upload a host arena + index (H2D copy,
 * device copy owned by the context).  Contract: pkt_off[k] % 16 == 0 and
 * pkt_off[k] + max(16, round_up(pkt_len[k], 16)) <= arena_bytes and pkt_len[k] <= 2^30 for every k (checked): every
 * payload, also an empty one, owns at least one readable 16-byte slot.  The bytes between a payload's
 * end and the end of its slot may hold anything; when they are 0x00 (as kmp_arena builds them -- checked
 * at load time, and cleared in the copy kmpgpu_load_arena makes) the streaming kernels take a payload's
 * end from the packet-start bitmap and never read the index on the scan path.
 * BEHIND THE LAST SLOT nothing is required: arena_bytes need only reach the end of the last slot
 * (pkt_off[k] + max(16, round_up(pkt_len[k], 16)) of the payload that lies last), no kernel reads a byte at or
 * behind that end, and whatever a caller keeps there -- the rest of a larger buffer of which the index is a
 * prefix view, a longer batch loaded earlier into the same device buffers -- never enters a count: a window
 * never leaves its payload (serial.c:193,198).  (The host library still leaves KMP_ARENA_SLACK zero bytes
 * there; the kernels do not depend on them.) */
int  kmpgpu_load_arena(kmpgpu_ctx *ctx, const uint8_t *arena, uint64_t arena_bytes,
                       const uint64_t *pkt_off, const uint32_t *pkt_len, uint64_t n_pkts);

/* Replaces the read loop AND the extraction phase (serial.c:115-141; openmp_data.c:128-147): upload the
 * raw capture file + the position of its frames (kmp_frames_from_pcap) and let the GPU apply the
 * dump_UDP_packet / dump_TCP_packet rules (packet_dumping.h:87-188) and pack the accepted payloads into
 * the context's arena.  tcp: 0 = UDP rule, 1 = TCP rule.  *n_payloads = payloads accepted. */
int  kmpgpu_load_frames(kmpgpu_ctx *ctx, const uint8_t *file_bytes, uint64_t file_nbytes, const uint64_t *frame_off,
                        const uint32_t *frame_caplen, uint64_t n_frames, int tcp, uint64_t *n_payloads);

/* The same in two steps, for a caller that keeps the copy engine busy (bin/openmp_task): _begin waits for the context's earlier passes,
 * then ENQUEUES the upload and the first extraction stage on the context's stream and returns; _finish waits for them, packs the
 * payloads and makes the new arena the context's current one.  Between the two the caller may begin a load on another context (its
 * upload queues up behind this one) or finish an earlier one.  The host buffers handed to _begin must stay valid and unchanged until
 * _finish has returned; scans of this context are only allowed again after _finish. */
int  kmpgpu_load_frames_begin(kmpgpu_ctx *ctx, const uint8_t *file_bytes, uint64_t file_nbytes, const uint64_t *frame_off,
                              const uint32_t *frame_caplen, uint64_t n_frames, int tcp);
int  kmpgpu_load_frames_finish(kmpgpu_ctx *ctx, uint64_t *n_payloads);
/* Between _begin and _finish: wait until the upload alone is through (the copy engine is free for the next context's). */
int  kmpgpu_load_frames_uploaded(kmpgpu_ctx *ctx);

/* Size the context's device buffers ahead of time for arenas of up to arena_bytes / n_pkts payloads and, when frame_bytes != 0, for
 * kmpgpu_load_frames calls of up to frame_bytes of capture / n_frames frames: a streamed capture (openmp_task.c:126-186) loads batch
 * after batch into the same buffers, and the first batch should not pay for a dozen device allocations.  Optional: every loader
 * grows what it needs. */
int  kmpgpu_reserve(kmpgpu_ctx *ctx, uint64_t arena_bytes, uint64_t n_pkts, uint64_t frame_bytes, uint64_t n_frames);

/* Same, for an arena already resident in device memory (borrowed; same contract, checked by a
 * device-side pass; an arena that is not packed is copied unless KMPGPU_OPT_REPACK is 0).  d_arena: uint8_t*, d_pkt_off: uint64_t*, d_pkt_len: uint32_t*.
 * IMMUTABILITY: the call derives state from the buffers -- packet-start bitmap, wavefront plan, uniform / packed
 * flags, the slot-padding check -- so arena AND index must stay unchanged for as long as they are attached.  A
 * device-resident batch ring that refills a buffer in place calls kmpgpu_attach_arena again after every refill (the
 * derived state is rebuilt by a few small kernels, no copy of the arena); scanning a rewritten buffer without it
 * counts against the OLD packet boundaries. */
int  kmpgpu_attach_arena(kmpgpu_ctx *ctx, const void *d_arena, uint64_t arena_bytes,
                         const void *d_pkt_off, const void *d_pkt_len, uint64_t n_pkts);

/* Replaces the hot loop serial.c:153-155 / openmp_data.c:157-175: counts_out[i] for every
 * pattern, in pattern order.  Synchronous; fills *t when non-NULL. */
int  kmpgpu_scan(kmpgpu_ctx *ctx, uint64_t *counts_out, kmpgpu_timing *t);

/* Asynchronous form: enqueue one full pass on the context's stream, no host synchronisation.
 * The counts (uint64_t[n_pat]) are written to d_counts_out, a caller-owned device buffer, or to
 * the context's own device buffer when d_counts_out is NULL.  That buffer is the operand of the
 * cross-GPU sum that replaces MPI_Reduce(local_string_count ...), mpi_dumping.c:202. */
int  kmpgpu_scan_enqueue(kmpgpu_ctx *ctx, void *d_counts_out);
/* Device address of the context's own counts buffer. */
void *kmpgpu_counts_device(kmpgpu_ctx *ctx);
/* Zero the context's own counts buffer (asynchronous, on the context's stream). */
int  kmpgpu_counts_reset(kmpgpu_ctx *ctx);
/* dst's counters += src's (both contexts on the same device, same patterns): the merge of contexts that share a GPU,
 * e.g. the two double-buffering contexts of a streamed capture (openmp_task.c:172-175).  Waits for src's stream, then
 * enqueues the addition on dst's. */
int  kmpgpu_counts_add(kmpgpu_ctx *dst, kmpgpu_ctx *src);
/* Timing of the context's last kmpgpu_load_arena / kmpgpu_load_frames / kmpgpu_scan. */
int  kmpgpu_last_timing(kmpgpu_ctx *ctx, kmpgpu_timing *t);
/* Wait for the context's stream and copy its own counts buffer to the host (uint64_t[n_pat]). */
int  kmpgpu_counts_read(kmpgpu_ctx *ctx, uint64_t *counts_out);
int  kmpgpu_sync(kmpgpu_ctx *ctx);

/* ---- the count reduce over GPUs: replaces MPI_Reduce(local_string_count, string_count, n, MPI_INT, MPI_SUM, 0, comm),
 * mpi_dumping.c:202 (and the scatter's rank/size bookkeeping, mpi_dumping.c:29-31) -- RCCL over xGMI.  librccl.so is
 * opened on the first call (no link-time dependency: single-GPU callers never load it).
 *
 * One rank per context, every context on its own device.
 *   kmpgpu_comm_init       all ranks live in THIS process (ncclCommInitAll): ctx[0..n_ctx) on n_ctx distinct devices;
 *   kmpgpu_comm_init_rank  one process per GPU (as mpirun starts mpi_dumping): rank `rank` of `n_ranks`, `unique_id`
 *                          (KMPGPU_COMM_ID_BYTES bytes) made once by kmpgpu_comm_unique_id and handed to every
 *                          rank by the launcher (file, environment, socket ...);
 *   kmpgpu_comm_allreduce_counts   enqueue ncclAllReduce(ncclUint64, ncclSum) in place over every local context's
 *                          counts buffer (kmpgpu_counts_device), on that context's stream, i.e. after the passes
 *                          enqueued so far (kmpgpu_scan_enqueue(ctx, NULL)); no host synchronisation: read the totals
 *                          with kmpgpu_counts_read afterwards (every rank holds them, like MPI_Allreduce).
 * All contexts of a communicator must hold the same number of patterns. */
#define KMPGPU_COMM_ID_BYTES 128
typedef struct kmpgpu_comm kmpgpu_comm;
int  kmpgpu_comm_init(kmpgpu_comm **comm, kmpgpu_ctx *const *ctx, int n_ctx);
int  kmpgpu_comm_unique_id(void *id_out);
int  kmpgpu_comm_init_rank(kmpgpu_comm **comm, kmpgpu_ctx *ctx, int n_ranks, int rank, const void *unique_id);
int  kmpgpu_comm_allreduce_counts(kmpgpu_comm *comm);
/* Lifetime: destroy the communicator BEFORE its contexts.  The other order is tolerated -- kmpgpu_destroy() of a context
 * that is still a rank waits for its stream and detaches it: kmpgpu_comm_allreduce_counts then fails with KMPGPU_ESTATE
 * and kmpgpu_comm_destroy only releases the RCCL handles -- but the peers of a detached rank must not enter another
 * collective.  A context belongs to at most one communicator.  Threads: kmpgpu_comm_init_rank may be called from one
 * thread per context at the same time (it blocks until every rank has joined); calls on ONE communicator are not
 * thread-safe.  While a communicator is being created the process's stdout (fd 1) points at stderr (RCCL's banner). */
void kmpgpu_comm_destroy(kmpgpu_comm *comm);
/* The device a context was created on. */
int  kmpgpu_device_of(kmpgpu_ctx *ctx);

/* Per-launch durations of the scan kernel, measured with HIP events on the launch stream.
 * begin(): start recording up to max_launches launches; end(): synchronise, write the
 * durations (ms) of the *n recorded launches, stop recording. */
int  kmpgpu_profile_begin(kmpgpu_ctx *ctx, uint32_t max_launches);
int  kmpgpu_profile_end(kmpgpu_ctx *ctx, float *ms_out, uint32_t *n);

/* Counts plus the matches themselves: every (packet, start offset, pattern) that counts (E_k follows KMPGPU_OPT_WHOLE_PAYLOAD: with
 * whole payloads the records behind a payload's first 0x00 appear), at most
 * cap of them written to out (host memory, unspecified order); *n_found is the total number found
 * (may exceed cap).  The pass writes its counts to a buffer of its own: the context's counters (a running total under
 * KMPGPU_OPT_ACCUMULATE, the result of a count reduce) stay as they are.  An arena that is scanned in place with slots
 * not back to back (KMPGPU_OPT_REPACK = 0) is packed on this call, once. */
int  kmpgpu_scan_offsets(kmpgpu_ctx *ctx, kmpgpu_match *out, uint64_t cap, uint64_t *n_found,
                         uint64_t *counts_out);

/* Which payloads hold which patterns (grep -l / grep -c per payload, an alert per packet, the filter in front of a packet
 * export -- kmpgpu_load_selected takes any[] or a row and compacts those payloads on the device): one bit per (pattern, payload), made on the device in one pass.  With c[k][i] the count defined at the top of
 * this file for payload k and pattern i (E_k as KMPGPU_OPT_WHOLE_PAYLOAD says, overlapping starts, KMPGPU_PAT_NOCASE where the
 * pattern carries it):
 *     hit[i][k]     = c[k][i] >= 1
 *     pkt_counts[i] = sum over k of hit[i][k]         (payloads that hold pattern i)
 *     any[k]        = OR over i of hit[i][k]          (payload k holds at least one pattern)
 *     counts[i]     = sum over k of c[k][i]           (exactly what kmpgpu_scan returns)
 * Duplicate patterns get identical rows, one per index; an empty payload never hits.
 * Layout: W = ceil(n_pkts / 64) words per row; payload k is bit (k & 63) of word (k >> 6), LSB first; row i of hits_out
 * starts at hits_out + i * W; the bits of index n_pkts and above are 0.  Every output may be NULL:
 * pkt_counts_out[n_pat], any_out[W], hits_out[n_pat * W], counts_out[n_pat].
 * Synchronous, on the context's stream; *t (may be NULL) gets kernel_ms (zeroing + scan launches + reduce), d2h_ms and
 * launches.  Preconditions and errors as kmpgpu_scan_offsets: streaming kernels only (KMPGPU_OPT_MODE 1 or KMPGPU_OPT_KERNEL
 * 1: KMPGPU_EINVAL), an arena kept in place with KMPGPU_OPT_REPACK = 0 is packed once, no patterns: KMPGPU_ESTATE; with
 * n_pkts == 0 every output is 0 and nothing is launched.  The pass writes to buffers of its own: the context's counters (a
 * running total under KMPGPU_OPT_ACCUMULATE, the result of a count reduce) stay as they are.
 * Cost: the scan kernels of kmpgpu_scan_offsets, which set the bit of a (pattern, payload) pair with one atomic OR per
 * distinct pair per wavefront and call instead of writing records, then one read of the bit matrix.  That matrix is device
 * memory owned by the context, n_pat x W x 8 bytes (97 patterns x 1 M payloads: 12 MB; 4 000 x 8 M: 4 GB), grown like the
 * other buffers, zeroed before every pass and freed by kmpgpu_destroy; when it cannot be allocated the call fails with
 * KMPGPU_ENOMEM / KMPGPU_EHIP and the context stays usable. */
int  kmpgpu_scan_packets(kmpgpu_ctx *ctx, uint64_t *pkt_counts_out /* [n_pat] or NULL */,
                         uint64_t *any_out /* [W] or NULL */, uint64_t *hits_out /* [n_pat * W] or NULL */,
                         uint64_t *counts_out /* [n_pat] or NULL */, kmpgpu_timing *t /* or NULL */);

/* Content rules: AND / NOT of patterns per payload, evaluated on the device behind the marking pass of kmpgpu_scan_packets (a
 * signature is several contents that must all be in one payload, often with one that must not be: "GET" and "/admin" and not
 * "Host: intranet"; grep -l a | xargs grep -l b | xargs grep -L c).  Only the per-rule results leave the device.
 * A rule is a non-empty list of terms; a term is a pattern index i < n_pat, | KMPGPU_RULE_NOT for a negated term.  With
 * hit[i][k] exactly as kmpgpu_scan_packets defines it (E_k as KMPGPU_OPT_WHOLE_PAYLOAD says, KMPGPU_PAT_NOCASE per pattern):
 *     rule_hit[r][k]     = AND over the positive terms i of hit[i][k]  AND  AND over the negated terms i of !hit[i][k]   (k < n_pkts)
 *     rule_pkt_counts[r] = sum over k of rule_hit[r][k]     (payloads that rule r matches)
 *     any[k]             = OR over r of rule_hit[r][k]      (payload k matches at least one rule)
 * So: a rule of negated terms only matches every payload that holds none of them, empty payloads included; i and !i in one rule
 * never matches; a term may repeat; rules may share patterns and may be identical, each rule index gets its own row.
 * Layout as kmpgpu_scan_packets: W = ceil(n_pkts / 64) words per row, payload k is bit (k & 63) of word (k >> 6), LSB first; row r
 * of rule_hits_out starts at rule_hits_out + r * W; the bits of index n_pkts and above are 0 in every output word, also for an
 * all-negated rule.
 *
 * kmpgpu_set_rules copies the rules and uploads them: rule r = terms[rule_off[r] .. rule_off[r + 1]), rule_off[n_rules + 1].  They
 * refer to the pattern set current at the call: no patterns set: KMPGPU_ESTATE; a later kmpgpu_set_patterns /
 * kmpgpu_set_patterns_flags drops them (the indices would mean something else), and so does every kmpgpu_set_relations.  rule_off[0] != 0, a decreasing rule_off, a rule
 * without terms or a term whose index is >= n_pat: KMPGPU_EINVAL, and the rules set before stay in force.  n_rules == 0 clears
 * the rules.
 *
 * kmpgpu_scan_rules: synchronous, on the context's stream.  The marking pass of kmpgpu_scan_packets (the same code: zeroing, scan
 * launches), then the rules kernel over the matrix instead of the pattern-level reduce; counts_out is what kmpgpu_scan returns.
 * Every output may be NULL: rule_pkt_counts_out[n_rules], any_out[W], rule_hits_out[n_rules * W], counts_out[n_pat].
 * Preconditions and errors as kmpgpu_scan_packets (streaming kernels only; an arena kept in place is packed once; with
 * n_pkts == 0 every output is 0 and nothing is launched; the context's counters stay as they are, also under
 * KMPGPU_OPT_ACCUMULATE); no rules set: KMPGPU_ESTATE.  *t (may be NULL): kernel_ms covers zeroing, scan launches and the rules
 * kernel, launches counts the rules kernel; under kmpgpu_profile_begin the rules kernel is recorded as the last launch.
 * kmpgpu_scan_packets returns the same before and after a kmpgpu_scan_rules on the context.
 * Cost: the rules kernel reads (sum of the rules' terms) x W x 8 bytes of the matrix (less where a payload word has already run
 * empty) and writes n_rules x W x 8.  Device memory, owned by the context next to the hit matrix, grown like the other buffers,
 * written or zeroed in full by every pass and freed by kmpgpu_destroy: with W2 = 2 * ceil(W / 2),
 *     (n_rules x W2  +  n_rules  +  W2) x 8 bytes      (100 rules x 1 M payloads: 12.5 MB; 4 000 x 8 M: 4 GB)
 * and 16 bytes per rule + 16 per four terms behind a rule's first two for the rules themselves.  When the rows cannot be allocated
 * the call fails with KMPGPU_ENOMEM / KMPGPU_EHIP and the context stays usable. */
#define KMPGPU_RULE_NOT 0x80000000u     /* term = pattern index | KMPGPU_RULE_NOT for a negated term */
int  kmpgpu_set_rules(kmpgpu_ctx *ctx, const uint32_t *rule_off /* [n_rules + 1], rule r = terms[rule_off[r] .. rule_off[r+1]) */,
                      const uint32_t *terms, uint32_t n_rules);
int  kmpgpu_scan_rules(kmpgpu_ctx *ctx, uint64_t *rule_pkt_counts_out /* [n_rules] or NULL */, uint64_t *any_out /* [W] or NULL */,
                       uint64_t *rule_hits_out /* [n_rules * W] or NULL */, uint64_t *counts_out /* [n_pat] or NULL: as kmpgpu_scan */,
                       kmpgpu_timing *t /* or NULL */);

/* Per-pattern offset windows: WHERE in its payload a match has to start ("GET " at offset 0, a magic number in the first 8 bytes, a
 * token only behind a 12-byte header; Snort / Suricata: offset, depth).  Pattern i gets a window [first_i, last_i] on the start offset
 * s of a match inside its payload; the default, and the state without windows, is [0, UINT32_MAX].  A match (k, s, i) that counts under
 * the rules at the top of this file (E_k as KMPGPU_OPT_WHOLE_PAYLOAD says, overlapping starts, KMPGPU_PAT_NOCASE per pattern) is IN
 * WINDOW iff
 *     first_i <= s <= last_i
 * Snort's `offset:o; depth:d` for a pattern of m bytes is first = o, last = o + d - m; a prefix anchor is [0, 0].  A window that lies
 * behind every payload's end never hits.  The window is on the payload's own offsets: a 0x00 in front of s takes the match away under
 * the default E_k and does not under KMPGPU_OPT_WHOLE_PAYLOAD, exactly as without windows.
 *
 * Who follows the windows:
 *     kmpgpu_scan_offsets   only in-window records are written, and *n_found is the number of in-window matches;
 *     kmpgpu_scan_packets   hit[i][k] = payload k has at least one in-window match of pattern i; pkt_counts and any follow from that hit;
 *     kmpgpu_scan_rules     rule_hit, rule_pkt_counts and any are defined over that hit; nothing else changes.
 * Duplicate patterns have a window each (their rows and records then differ): this is how one byte string is used with two windows,
 * in two rules or in one.
 * Who does NOT: kmpgpu_scan and kmpgpu_scan_enqueue do not look at windows, and counts_out of the three calls above stays exactly
 * what kmpgpu_scan returns -- every match, in window or not.  So with windows set pkt_counts[i] == 0 no longer implies
 * counts[i] == 0, *n_found may be smaller than the sum of counts_out, and the context's own counters (KMPGPU_OPT_ACCUMULATE) are as
 * untouched as before.  Windowed counts and windows relative to a payload's end do not exist; a window between two
 * patterns (distance / within) is a relation, kmpgpu_set_relations below, and a match has to be in window to enter one.
 * With no windows set, or with every window the default, every output of every call is bit-identical to what it is without this
 * call, and the kernels run what they run without it.
 *
 * kmpgpu_set_windows copies first[n_pat], last[n_pat] and uploads them (8 bytes per pattern of device memory, owned by the context,
 * uploaded on its stream, freed by kmpgpu_destroy).  The windows belong to the pattern set current at the call: no patterns set:
 * KMPGPU_ESTATE; n_pat different from the context's pattern count, first[i] > last[i] for some i, or a NULL array: KMPGPU_EINVAL;
 * after any error the windows set before stay in force.  n_pat == 0 clears the windows (first and last are ignored and may be
 * NULL).  A later kmpgpu_set_patterns / kmpgpu_set_patterns_flags drops them, as it drops the rules.  Windows are pass state:
 * they may be set, changed and cleared between two passes of one context with nothing reloaded or re-attached, and rules set
 * earlier stay valid -- they name pattern indices, the windows change what a hit is.
 * Cost (measured, DESIGN.md §3.13, profiles/windows.txt): nothing for kmpgpu_scan / kmpgpu_scan_enqueue, whose kernels are the
 * code they were; a marking pass without windows takes the time it took within the run-to-run spread; with a window on every
 * pattern the pass pays for the filter in its emitters -- with windows that drop nothing +4 % for one 16-byte pattern, +9 % for
 * 97 tokens in the fused pass (a per-match load of the window), +25 % on text that matches at every offset -- and gets faster
 * where the windows drop matches (97 tokens with [0, 63]: 0.71 of the time without windows). */
int  kmpgpu_set_windows(kmpgpu_ctx *ctx, const uint32_t *first /* [n_pat] */, const uint32_t *last /* [n_pat] */, uint32_t n_pat);

/* Relations between two patterns: HOW FAR the start of one lies behind the end of the other ("Host:" at most 20 bytes behind the end of
 * "GET "; Snort / Suricata: distance, within), decided on the device behind the marking pass of kmpgpu_scan_packets.  A rule "a and b"
 * fires on any payload that holds both patterns anywhere; relation q = {a, b, dmin, dmax} fires where two of their matches lie as asked.
 * Write (k, s, i) for a match of pattern i at start offset s of payload k that counts under the rules at the top of this file (E_k as
 * KMPGPU_OPT_WHOLE_PAYLOAD says, overlapping starts, KMPGPU_PAT_NOCASE per pattern) AND is in window (kmpgpu_set_windows) -- exactly
 * the matches that set hit[i][k] of kmpgpu_scan_packets.  With m_a the length of pattern a:
 *     rel_hit[q][k]     = there are matches (k, sa, a) and (k, sb, b) with  dmin <= (int64)sb - ((int64)sa + m_a) <= dmax
 *     rel_pkt_counts[q] = sum over k of rel_hit[q][k]      (payloads in which relation q holds)
 *     any[k]            = OR over q of rel_hit[q][k]
 *     counts[i]         = exactly what kmpgpu_scan returns, as in the sibling calls (every match, in window or not)
 * dmin == INT32_MIN: no lower bound; dmax == INT32_MAX: no upper bound.  Snort's `distance:d` is dmin = d; `within:w` behind it is
 * dmax = d + w - m_b (b has to END inside the w bytes), without a distance d = 0.  Negative values put b in front of a or let the two
 * overlap (sb = sa is -m_a).  a == b is allowed and taken literally: two occurrences of one pattern, or one match paired with itself
 * where -m_a lies in [dmin, dmax].  Relations may share patterns and may be identical; each index gets its own row.
 * Layout as kmpgpu_scan_packets: W = ceil(n_pkts / 64) words per row, payload k is bit (k & 63) of word (k >> 6), LSB first; row q of
 * rel_hits_out starts at rel_hits_out + q * W; the bits of index n_pkts and above are 0 in every output word.
 *
 * Relations as rule terms: while relations are set, relation q is term index n_pat + q of kmpgpu_set_rules and may carry
 * KMPGPU_RULE_NOT; the bound that kmpgpu_set_rules checks is n_pat + n_rel (n_pat with none set), and kmpgpu_scan_rules runs the relation
 * kernel between its marking pass and its rules kernel -- only then.  n_pat + n_rel < 2^31.
 * NOT A CHAIN: every relation is decided on its own.  A rule of rel(a, b) and rel(b, c) asks for some pair (a, b) and some pair (b, c);
 * the two b need not be the same match.  Snort's chained contents (each relative to the match before) are a chain: kmpgpu_set_chains
 * below.
 *
 * kmpgpu_set_relations copies rel[n_rel] and uploads it (16 bytes per relation of device memory, owned by the context, freed by
 * kmpgpu_destroy).  The relations belong to the pattern set current at the call: no patterns set: KMPGPU_ESTATE; a later
 * kmpgpu_set_patterns / kmpgpu_set_patterns_flags drops them, as it drops rules and windows.  a or b >= n_pat, dmin > dmax, rel == NULL
 * with n_rel > 0, n_pat + n_rel >= 2^31: KMPGPU_EINVAL, and the relations and rules set before stay in force.  EVERY successful call
 * drops the rules, n_rel == 0 (which clears the relations; rel may be NULL) included: the rows their terms name have changed.  So the
 * order is patterns, relations, rules.  Windows and KMPGPU_OPT_WHOLE_PAYLOAD stay pass state: they may change between two passes with
 * nothing set again, and the relations follow them.
 *
 * kmpgpu_scan_relations: synchronous, on the context's stream.  The marking pass of kmpgpu_scan_packets (the same code), then the
 * relation kernel instead of the pattern-level reduce.  Every output may be NULL: rel_pkt_counts_out[n_rel], any_out[W],
 * rel_hits_out[n_rel * W], counts_out[n_pat].  Preconditions and errors as kmpgpu_scan_packets (streaming kernels only; an arena kept
 * in place is packed once; with n_pkts == 0 every output is 0 and nothing is launched; the context's counters stay as they are); no
 * relations set: KMPGPU_ESTATE.  *t (may be NULL): kernel_ms covers zeroing, scan launches and the relation kernel, launches counts
 * it; under kmpgpu_profile_begin it is recorded behind the scan launches (in kmpgpu_scan_rules: in front of the rules kernel).
 * With no relations set every output of every other call is bit-identical to what it is without these two calls, with the same
 * launches and device buffers.
 * Cost (the figures of tools/relations.py go to profiles/relations.txt): the relations are n_rel further rows of the hit matrix, (n_rel x W2 + n_rel)
 * x 8 bytes, zeroed with it.  The kernel reads two words of the matrix per (relation, 64 payloads) and then only the payloads that
 * hold both patterns: one wavefront per such payload finds E_k and sweeps the text 64 start offsets at a time, with no memory that
 * grows with the payload.  Few candidates: a pass over the matrix.  Every payload a candidate of every relation: n_rel reads of the
 * arena, a wavefront per payload -- the dense case of §3.15. */
typedef struct kmpgpu_relation {
    uint32_t a, b;            /* pattern indices (file order); b is measured from the END of a                 */
    int32_t  dmin, dmax;      /* dmin <= start of b - end of a <= dmax; INT32_MIN / INT32_MAX: unbounded side */
} kmpgpu_relation;
int  kmpgpu_set_relations(kmpgpu_ctx *ctx, const kmpgpu_relation *rel /* [n_rel] */, uint32_t n_rel);
int  kmpgpu_scan_relations(kmpgpu_ctx *ctx, uint64_t *rel_pkt_counts_out /* [n_rel] or NULL */, uint64_t *any_out /* [W] or NULL */,
                           uint64_t *rel_hits_out /* [n_rel * W] or NULL */, uint64_t *counts_out /* [n_pat] or NULL: as kmpgpu_scan */,
                           kmpgpu_timing *t /* or NULL */);

/* Content chains: every content measured from THE MATCH BEFORE IT (Snort / Suricata: content:"A"; content:"B"; distance:0; within:10;
 * content:"C"; distance:5; -- C is measured from the same B that was measured from A), decided on the device behind the marking pass of
 * kmpgpu_scan_packets.  A rule of rel(A, B) and rel(B, C) asks for less: its two B may be different matches, and on repetitive traffic
 * (a header name twice) it fires where the signature does not.
 * A chain is 2 .. KMPGPU_CHAIN_MAX contents p_0 .. p_{n-1}, each a pattern index; links j = 1 .. n-1 carry (dmin_j, dmax_j).  With
 * (k, s, i) a match exactly as relations define it (it counts under the rules at the top of this file, E_k as KMPGPU_OPT_WHOLE_PAYLOAD
 * says, overlapping starts, KMPGPU_PAT_NOCASE per pattern, AND it is in window) and m_i the length of pattern i:
 *     chain_hit[c][k]     = there are matches (k, s_0, p_0) .. (k, s_{n-1}, p_{n-1}) with
 *                           dmin_j <= (int64)s_j - ((int64)s_{j-1} + m_{p_{j-1}}) <= dmax_j   for every j = 1 .. n-1
 *     chain_pkt_counts[c] = sum over k of chain_hit[c][k]
 *     any[k]              = OR over c of chain_hit[c][k]
 *     counts[i]           = exactly what kmpgpu_scan returns, as in the sibling calls
 * dmin == INT32_MIN / dmax == INT32_MAX: that side is open, as for relations.  The definition is existential over all tuples, not
 * greedy: the first B behind A may be out of reach of every C while a later one serves.  A pattern may repeat inside a chain and is
 * taken literally: a, a, a is three occurrences, or fewer where a negative distance lets a match pair with itself.  A chain of two
 * contents is bit-identical to the relation {p_0, p_1, dmin_1, dmax_1}.  Chains may share patterns and may be identical; each index
 * gets its own row.  Layout as kmpgpu_scan_packets: W = ceil(n_pkts / 64) words per row, row c of chain_hits_out starts at
 * chain_hits_out + c * W; the bits of index n_pkts and above are 0 in every output word.
 *
 * kmpgpu_set_chains copies and uploads the chains: chain c = links[chain_off[c] .. chain_off[c + 1]), chain_off[n_chains + 1].  Its first
 * link names p_0 and must carry INT32_MIN / INT32_MAX: it is relative to nothing (a position constraint on p_0 is a window).  The chains
 * belong to the pattern set current at the call: no patterns set: KMPGPU_ESTATE; a later kmpgpu_set_patterns /
 * kmpgpu_set_patterns_flags drops them, as it drops rules, windows and relations; kmpgpu_set_relations keeps them (they name patterns,
 * not rows).  chain_off[0] != 0, a decreasing chain_off, a chain of fewer than 2 or more than KMPGPU_CHAIN_MAX links, a pattern index
 * >= n_pat, dmin > dmax, bounds on a first link, a NULL array with n_chains > 0, n_pat + n_rel + n_chains >= 2^31: KMPGPU_EINVAL, and the
 * chains and rules set before stay in force.  n_chains == 0 clears the chains (the arrays may be NULL).  EVERY successful call drops the
 * rules: the rows their terms name have changed.  So the order is patterns, relations, chains, rules.  (A kmpgpu_set_relations that
 * would push n_pat + n_rel + n_chains to 2^31 is refused in the same way.)
 *
 * Chains as rule terms: while chains are set, chain c is term index n_pat + n_rel + c of kmpgpu_set_rules and may carry KMPGPU_RULE_NOT;
 * the bound that kmpgpu_set_rules checks is n_pat + n_rel + n_chains, and kmpgpu_scan_rules runs the relation kernel where relations are
 * set, then the chain kernel where chains are set, then the rules kernel.
 *
 * kmpgpu_scan_chains: synchronous, on the context's stream.  The marking pass of kmpgpu_scan_packets, then the chain kernel instead of
 * the pattern-level reduce.  Every output may be NULL: chain_pkt_counts_out[n_chains], any_out[W], chain_hits_out[n_chains * W],
 * counts_out[n_pat].  Preconditions and errors as kmpgpu_scan_packets (streaming kernels only; an arena kept in place is packed once;
 * with n_pkts == 0 every output is 0 and nothing is launched; the context's counters stay as they are); no chains set: KMPGPU_ESTATE.
 * *t (may be NULL): kernel_ms covers zeroing, scan launches and the chain kernel, launches counts it; under kmpgpu_profile_begin it is
 * recorded behind the scan launches (in kmpgpu_scan_rules: between the relation kernel and the rules kernel).
 * With no chains set every output of every other call is bit-identical to what it is without these two calls, with the same launches
 * and device buffers.
 * Cost (the figures of tools/chains.py go to profiles/chains.txt): the chains are n_chains further rows of the hit
 * matrix, (n_chains x W2 + n_chains) x 8 bytes, zeroed with it, and KMPGPU_CHAIN_MAX x 16 bytes per chain for the chains themselves.
 * The kernel reads n words of the matrix per (chain, 64 payloads) and then only the payloads that hold every content: one wavefront
 * per such payload sweeps the text 64 offsets at a time with one carried position per link and no memory that grows with the payload;
 * a link with an open side widens the sweep by about twice the payload's length. */
#define KMPGPU_CHAIN_MAX 8
typedef struct kmpgpu_chain_link {
    uint32_t pattern;         /* pattern index (file order)                                                                   */
    int32_t  dmin, dmax;      /* dmin <= start of this content - end of the one before <= dmax; first link: INT32_MIN, INT32_MAX */
} kmpgpu_chain_link;
int  kmpgpu_set_chains(kmpgpu_ctx *ctx, const uint32_t *chain_off /* [n_chains + 1] */, const kmpgpu_chain_link *links, uint32_t n_chains);
int  kmpgpu_scan_chains(kmpgpu_ctx *ctx, uint64_t *chain_pkt_counts_out /* [n_chains] or NULL */, uint64_t *any_out /* [W] or NULL */,
                        uint64_t *chain_hits_out /* [n_chains * W] or NULL */, uint64_t *counts_out /* [n_pat] or NULL: as kmpgpu_scan */,
                        kmpgpu_timing *t /* or NULL */);

/* Header predicates: the rule HEADER of a signature -- "alert udp 10.0.0.0/8 any -> any 53", with dsize -- as a fifth kind of row
 * of the hit matrix, beside patterns, relations and chains.  A predicate is decided from 16 bytes of per-payload metadata and the payload's
 * length in the index, not from the text.
 *
 * Metadata.  kmpgpu_pkt_meta is what the extractors saw on their way to the payload, in payload order, one record per payload.  With p the
 * frame: src_ip = p[26]<<24 | p[27]<<16 | p[28]<<8 | p[29], dst_ip likewise from p[30..33] (host-order integers); with
 * T = 14 + ((p[14] & 0x0F) << 2): src_port = p[T]<<8 | p[T+1], dst_port = p[T+2]<<8 | p[T+3]; proto = p[23]; reserved 0.  The byte
 * positions are the extractors' own: no EtherType or IP-version test, the IHL from the low nibble of byte 14 -- the metadata follows the
 * reference's quirks (in tcp mode its extractor does not test the protocol byte: proto says what a payload really is).  For every frame
 * either extractor accepts these bytes lie inside caplen; a rejected frame has no payload and no metadata.
 * Where it comes from: kmpgpu_load_frames / _begin under KMPGPU_OPT_KEEP_META = 1 (one further kernel behind the index scatter; with 0 the
 * load is what it is without the option and leaves no metadata), kmpgpu_set_meta for an arena that came through kmpgpu_load_arena /
 * kmpgpu_attach_arena, and kmpgpu_load_selected, which hands dst the metadata of the selected payloads, in order, whenever src has some
 * (one further kernel: launches 6, or 4 when nothing is selected; without metadata on src 5 / 3 as before).
 * Lifetime: metadata belongs to the arena.  Every loader that puts a new arena into the context drops it (kmpgpu_load_arena,
 * kmpgpu_attach_arena, kmpgpu_load_frames without the option, kmpgpu_load_selected as dst from a src without metadata); it survives the
 * on-device repack (which keeps payload order), kmpgpu_set_patterns and every option.
 * kmpgpu_set_meta copies meta[n_pkts] (on_device == 0: host memory; == 1: device memory on the context's device, 4-byte aligned; any other
 * value: KMPGPU_EINVAL) into a buffer the context owns.  n_pkts must equal the context's payload count: otherwise KMPGPU_EINVAL; no
 * arena: KMPGPU_ESTATE; n_pkts == 0 with a NULL pointer clears the metadata.  After an error the metadata that was there stays.
 * kmpgpu_meta_download copies the records to out[cap] and leaves their number in *n (either may be NULL); cap below the payload count
 * with out given: KMPGPU_EINVAL; no metadata: KMPGPU_ESTATE.
 *
 * Predicates.  With M = meta[k] and L_k the payload's length in the index (Snort's dsize; whatever KMPGPU_OPT_WHOLE_PAYLOAD says):
 *     dir(s, d, sp, dp) = (s & src_mask) == (src_ip & src_mask) && (d & dst_mask) == (dst_ip & dst_mask)
 *                         && sport_lo <= sp <= sport_hi && dport_lo <= dp <= dport_hi
 *     hdr_hit[q][k]     = ((flags & KMPGPU_HDR_ANY_PROTO) || M.proto == proto) && len_lo <= L_k <= len_hi
 *                         && (dir(M.src_ip, M.dst_ip, M.src_port, M.dst_port)
 *                             || ((flags & KMPGPU_HDR_BIDIR) && dir(M.dst_ip, M.src_ip, M.dst_port, M.src_port)))
 *     hdr_pkt_counts[q] = sum over k of hdr_hit[q][k]
 *     any[k]            = OR over q of hdr_hit[q][k]
 *     counts[i]         = exactly what kmpgpu_scan returns, as in the sibling calls
 * Masks are taken literally: /0 is mask 0, a non-contiguous mask is allowed.  An empty payload has metadata and can hit.  Layout as
 * kmpgpu_scan_packets: W = ceil(n_pkts / 64) words per row, row q of hdr_hits_out starts at hdr_hits_out + q * W; the bits of index
 * n_pkts and above are 0 in every output word.
 *
 * kmpgpu_set_headers copies and uploads the predicates.  They belong to the pattern set current at the call: no patterns set:
 * KMPGPU_ESTATE; a later kmpgpu_set_patterns / kmpgpu_set_patterns_flags drops them with everything else; kmpgpu_set_relations and
 * kmpgpu_set_chains keep them (and drop the rules, as they always do).  sport_lo > sport_hi, dport_lo > dport_hi, len_lo > len_hi, an
 * unknown flag bit, reserved != 0, a NULL array with n_hdr > 0, n_pat + n_rel + n_chains + n_hdr >= 2^31: KMPGPU_EINVAL, and the
 * predicates and rules set before stay in force.  n_hdr == 0 clears them (the array may be NULL).  EVERY successful call drops the rules:
 * the rows their terms name have changed.  So the order is patterns, relations, chains, headers, (byte tests,) rules.
 *
 * Headers as rule terms: predicate q is row n_pat + n_rel + n_chains + q of the hit matrix and term index n_pat + n_rel + n_chains + q of
 * kmpgpu_set_rules, with or without KMPGPU_RULE_NOT; kmpgpu_scan_rules and kmpgpu_scan_alerts(KMPGPU_ALERT_RULES) run the header kernel
 * behind the chain kernel and in front of the rules kernel whenever predicates are set (one launch; under kmpgpu_profile_begin it is
 * recorded in that place).  kmpgpu_scan_alerts has no family of its own for them: the rules family is how header hits reach the list.
 *
 * kmpgpu_scan_headers: synchronous, on the context's stream.  The marking pass of kmpgpu_scan_packets, then the header kernel instead of
 * the pattern-level reduce.  Every output may be NULL: hdr_pkt_counts_out[n_hdr], any_out[W], hdr_hits_out[n_hdr * W], counts_out[n_pat].
 * Preconditions and errors as kmpgpu_scan_packets; no predicates set: KMPGPU_ESTATE.  Predicates set but no metadata on the context:
 * KMPGPU_ESTATE ("no packet metadata") from kmpgpu_scan_headers, kmpgpu_scan_rules and kmpgpu_scan_alerts(KMPGPU_ALERT_RULES) alike, with
 * nothing launched; the context stays usable.
 * With no predicates set and KMPGPU_OPT_KEEP_META at 0 every output of every other call is bit-identical to what it is without these
 * calls, with the same launches and device buffers.
 * Cost (the figures of tools/headers.py go to profiles/headers.txt): n_hdr further rows of the hit matrix,
 * (n_hdr x W2 + n_hdr) x 8 bytes, zeroed with it, 48 bytes per predicate, 16 bytes of metadata per payload.  The kernel reads 20 bytes
 * per payload once, whatever n_hdr is, and writes every row in 16-byte pieces. */
typedef struct kmpgpu_pkt_meta {   /* 16 bytes; kmp_pkt_meta in kmphost.h has the same layout */
    uint32_t src_ip, dst_ip;       /* host-order integers */
    uint16_t src_port, dst_port;
    uint8_t  proto;                /* frame byte 23 */
    uint8_t  reserved[3];          /* 0 */
} kmpgpu_pkt_meta;
#define KMPGPU_HDR_ANY_PROTO 1u
#define KMPGPU_HDR_BIDIR     2u
typedef struct kmpgpu_header {
    uint32_t src_ip, src_mask, dst_ip, dst_mask;
    uint16_t sport_lo, sport_hi, dport_lo, dport_hi;
    uint32_t len_lo, len_hi;       /* on L_k, the payload's length in the index (Snort's dsize) */
    uint8_t  proto, flags;         /* flags: KMPGPU_HDR_* */
    uint16_t reserved;             /* 0 */
} kmpgpu_header;
int  kmpgpu_set_meta(kmpgpu_ctx *ctx, const void *meta /* kmpgpu_pkt_meta[n_pkts] */, uint64_t n_pkts, int on_device);
int  kmpgpu_meta_download(kmpgpu_ctx *ctx, kmpgpu_pkt_meta *out /* [cap] or NULL */, uint64_t cap, uint64_t *n /* or NULL */);
int  kmpgpu_set_headers(kmpgpu_ctx *ctx, const kmpgpu_header *h /* [n_hdr] */, uint32_t n_hdr);
int  kmpgpu_scan_headers(kmpgpu_ctx *ctx, uint64_t *hdr_pkt_counts_out /* [n_hdr] or NULL */, uint64_t *any_out /* [W] or NULL */,
                         uint64_t *hdr_hits_out /* [n_hdr * W] or NULL */, uint64_t *counts_out /* [n_pat] or NULL: as kmpgpu_scan */,
                         kmpgpu_timing *t /* or NULL */);

/* Byte tests: what signatures for binary protocols are built from -- read 1 to 4 bytes at a position, take them as an unsigned integer,
 * mask, compare (Snort: byte_test) -- as a sixth kind of row of the hit matrix, behind the header predicates'.  "Is the QR bit of a DNS
 * message set": 2 bytes at 2, mask 0x8000, NE, 0.  A pattern cannot say that: the field is a range or a bit, not a byte string.
 *
 * With E_k the payload's text end as everywhere else (min(L_k, first 0x00) under the default rule, L_k under KMPGPU_OPT_WHOLE_PAYLOAD):
 *     field(k, pos)     = the integer formed from bytes pos .. pos + nbytes - 1 of payload k, big-endian (network order) unless
 *                         KMPGPU_BT_LITTLE; defined only for 0 <= pos and pos + nbytes <= E_k: no byte at or behind E_k is ever part
 *                         of a field
 *     holds(f)          = ((f & mask) op value), unsigned 32-bit
 *     absolute test:      bt_hit[q][k] = field(k, offset) is defined && holds(field(k, offset))
 *     relative test:      bt_hit[q][k] = there is a match (k, s, anchor) such that field(k, s + m_anchor + offset) is defined and holds
 *     bt_pkt_counts[q]  = sum over k of bt_hit[q][k]
 *     any[k]            = OR over q of bt_hit[q][k]
 *     counts[i]         = exactly what kmpgpu_scan returns, as in the sibling calls
 * A match is what the marking pass marks, as the relations define it: in its window, nocase per pattern, overlapping starts; the test is
 * existential over ALL matches of the anchor, not only the first.  offset of a relative test has any sign: a negative one reaches into
 * the match or in front of it.  Out of reach is FALSE, not undecided: a field that cannot lie inside the text makes the test false, so a
 * negated term of a rule fires on a payload that is too short.  The field's bytes always come from the original arena, never from the
 * folded copy, also where the anchor is a nocase pattern compared in the fold.
 * No further operators: Snort's isdataat:N is {nbytes 1, KMPGPU_BT_GE, value 0} at offset N (a byte exists there), the bit test "&" is
 * {mask = bits, KMPGPU_BT_NE, value 0}.  Duplicate tests are allowed, each gets its row.  Layout as kmpgpu_scan_packets:
 * W = ceil(n_pkts / 64) words per row, LSB first, row q of bt_hits_out at bt_hits_out + q * W, the bits of index n_pkts and above 0.
 *
 * kmpgpu_set_bytetests copies and uploads the tests.  They belong to the pattern set current at the call: no patterns set: KMPGPU_ESTATE;
 * a later kmpgpu_set_patterns / kmpgpu_set_patterns_flags drops them with everything else; kmpgpu_set_relations, kmpgpu_set_chains and
 * kmpgpu_set_headers keep them (they name patterns, not rows) and count n_bt in their 2^31 bound.  nbytes outside 1..4, an unknown op or
 * flag bit, reserved != 0, anchor >= n_pat of a relative test, anchor != 0 or offset < 0 of an absolute one, a NULL array with n_bt > 0,
 * n_pat + n_rel + n_chains + n_hdr + n_bt >= 2^31: KMPGPU_EINVAL, and everything set before stays in force.  n_bt == 0 clears them (the
 * array may be NULL).  EVERY successful call drops the rules.  So the order is patterns, relations, chains, headers, byte tests, rules.
 * Windows and KMPGPU_OPT_WHOLE_PAYLOAD stay pass state: the tests follow what is set when a pass runs.
 *
 * Byte tests as rule terms: test q is row n_pat + n_rel + n_chains + n_hdr + q of the hit matrix and term index
 * n_pat + n_rel + n_chains + n_hdr + q of kmpgpu_set_rules, with or without KMPGPU_RULE_NOT; kmpgpu_scan_rules and
 * kmpgpu_scan_alerts(KMPGPU_ALERT_RULES) run the byte-test kernels (one for the absolute tests, one for the relative ones, each only
 * where there are some) behind the header kernel and in front of the rules kernel.  kmpgpu_scan_flows folds their rows under
 * KMPGPU_FLOW_SCOPE_FLOW as it folds every term row.  There is no KMPGPU_ALERT_* family for them: as with the header predicates the rules
 * family is how their hits reach the alert list and the flows.  A test sees one payload: none across a flow seam (kmpgpu_load_seams).
 *
 * kmpgpu_scan_bytetests: synchronous, on the context's stream.  The marking pass of kmpgpu_scan_packets, then the byte-test kernels
 * instead of the pattern-level reduce.  Every output may be NULL: bt_pkt_counts_out[n_bt], any_out[W], bt_hits_out[n_bt * W],
 * counts_out[n_pat].  Preconditions and errors as kmpgpu_scan_packets; no byte tests set: KMPGPU_ESTATE.
 * With no byte tests set every output of every other call is bit-identical to what it is without these calls, with the same launches and
 * device buffers.
 * Cost (the figures of tools/bytetests.py go to profiles/bytetests.txt): n_bt further rows of the hit matrix,
 * (n_bt x W2 + n_bt) x 8 bytes, zeroed with it, 32 bytes per test.  The absolute kernel reads 12 bytes of index per payload, under the
 * strlen rule the first min(L_k, H) bytes (H = the largest offset + nbytes) up to the first 0x00, and 4 or 8 bytes per (payload, test);
 * the relative kernel reads only the payloads that hold the anchor. */
#define KMPGPU_BT_RELATIVE 1u     /* measured from the END of a match of pattern `anchor` */
#define KMPGPU_BT_LITTLE   2u     /* little-endian; default big-endian (network order) */
enum { KMPGPU_BT_EQ, KMPGPU_BT_NE, KMPGPU_BT_LT, KMPGPU_BT_GT, KMPGPU_BT_LE, KMPGPU_BT_GE };
typedef struct kmpgpu_bytetest {
    uint32_t anchor;               /* pattern index; read only with KMPGPU_BT_RELATIVE, else must be 0 */
    int32_t  offset;               /* absolute: from the payload's first byte, >= 0; relative: from the anchor match's end, any sign */
    uint32_t mask, value;          /* ((field & mask) op value), unsigned 32-bit */
    uint8_t  nbytes, op, flags, reserved;   /* nbytes 1..4 */
} kmpgpu_bytetest;
int  kmpgpu_set_bytetests(kmpgpu_ctx *ctx, const kmpgpu_bytetest *bt /* [n_bt] */, uint32_t n_bt);
int  kmpgpu_scan_bytetests(kmpgpu_ctx *ctx, uint64_t *bt_pkt_counts_out /* [n_bt] or NULL */, uint64_t *any_out /* [W] or NULL */,
                           uint64_t *bt_hits_out /* [n_bt * W] or NULL */, uint64_t *counts_out /* [n_pat] or NULL: as kmpgpu_scan */,
                           kmpgpu_timing *t /* or NULL */);

/* Regex rows: expressions of byte classes and repeats (the linear part of a PCRE content), decided per payload, as a seventh kind of row of the
 * hit matrix, behind the byte tests'.  "User-Agent: followed by at least 40 non-newline bytes", "a run of 8 or more digits", "= with optional
 * blanks around it", "a line that is only hex digits": what no fixed byte string, relation, chain or byte test says.
 *
 * The dialect.  An expression is a byte string of at least one element, with an optional leading ^ and an optional trailing $.
 *   Elements, each one byte class:
 *     a literal byte    any byte other than 0x00 and the metacharacters \ . [ ] ( ) { } * + ? | ^ $; the bytes 0x80 .. 0xFF are literals
 *     an escape         \xHH, \n \r \t \f \v, \0 not followed by a digit, and \ followed by an ASCII punctuation byte, which is that byte
 *     a class escape    \d \D \w \W \s \S in Python's ASCII meaning on bytes: \s is {9 .. 13, 32}, \w is [A-Za-z0-9_]
 *     the dot           every byte but 0x0A; with KMPGPU_RX_DOTALL every byte
 *     a bracket class   [...] and [^...] of single bytes, escapes as above, ranges a-z whose endpoints are single bytes, and class escapes;
 *                       ] and \ inside a class are written escaped; - is a literal when it is first, last or escaped; an empty class is
 *                       refused
 *   Quantifiers, each behind one element: ? * + {n} {n,} {n,m} with n <= m and m >= 1.
 *   Refused with KMPGPU_EINVAL, the message naming the expression's index and the byte position ("expression Q: position P: ..."), everything
 *   set before staying in force: ( ) | (reserved for later), a quantifier on nothing or on a quantifier (a**, a+?), {,m}, ^ anywhere but
 *   first, $ anywhere but last, a raw 0x00, an unknown letter escape, a bad range, an unterminated class or brace, zero elements, more
 *   than KMPGPU_RX_MAX_POSITIONS positions.
 *   Positions: C{n,m} is n mandatory positions and m - n optional ones, C{n,} n - 1 mandatory ones and one mandatory repeatable one (for
 *   n = 0 it is C*), C* one optional repeatable position, C+ one repeatable one, C? one optional one, a bare element one mandatory one.
 *   KMPGPU_RX_NOCASE: the listed set of a literal or class is closed under ASCII case BEFORE a [^...] negates it: [^a] does not match A.
 *
 * The meaning.  With E_k the payload's text end as everywhere else (its first 0x00 under the default rule, L_k under
 * KMPGPU_OPT_WHOLE_PAYLOAD):
 *     rx_hit[q][k]     = (no gate || hit[gate_q][k])
 *                        && there are 0 <= s <= e <= E_k with payload_k[s:e] in L(expr_q),
 *                           s == 0 where the expression starts with ^, e == E_k where it ends with $
 *     rx_pkt_counts[q] = sum over k of rx_hit[q][k]
 *     any[k]           = OR over q of rx_hit[q][k]
 *     counts[i]        = exactly what kmpgpu_scan returns
 * $ is the text end alone (Python's \Z, not Python's $, which also matches in front of a final newline).  An expression that matches the
 * empty string (x*) hits every payload, the empty one included.  Under KMPGPU_OPT_WHOLE_PAYLOAD a 0x00 is a text byte that ., \x00, \D,
 * [^a] and the like match; under the default rule no byte at or behind E_k is seen.  hit[gate][k] is the bit of kmpgpu_scan_packets: in
 * the pattern's window, nocase per pattern.  The gate (KMPGPU_RX_GATED, gate[q] a pattern index) is a cost device with a defined meaning --
 * the expression is looked at only in payloads that hold pattern gate[q], Snort's fast pattern -- and no position: the expression is not
 * relative to the match.  The yardstick is Python's re on bytes: re.compile(expr with a trailing $ rewritten to \Z, re.I / re.S per
 * flag).search(payload[:E_k]) is not None, and-ed with the gate's row (tests/regex_model.py).
 *
 * kmpgpu_set_regexes compiles, copies and uploads the expressions.  They belong to the pattern set current at the call: no patterns set:
 * KMPGPU_ESTATE; a later kmpgpu_set_patterns / kmpgpu_set_patterns_flags drops them with everything else; kmpgpu_set_relations, _chains,
 * _headers and _bytetests keep them and count n_rx in their 2^31 bound.  An expression outside the dialect, an unknown flag bit,
 * gate[q] >= n_pat with KMPGPU_RX_GATED, gate[q] != 0 without it, a NULL array with n_rx > 0 (flags NULL: all 0, gate NULL: none gated),
 * n_pat + n_rel + n_chains + n_hdr + n_bt + n_rx >= 2^31: KMPGPU_EINVAL, and everything set before stays in force.  n_rx == 0 clears them.
 * EVERY successful call drops the rules.  So the order is patterns, relations, chains, headers, byte tests, regexes, rules.  Windows and
 * KMPGPU_OPT_WHOLE_PAYLOAD stay pass state: the expressions follow what is set when a pass runs.
 *
 * Expressions as rule terms: expression q is row n_pat + n_rel + n_chains + n_hdr + n_bt + q of the hit matrix and term index
 * n_pat + n_rel + n_chains + n_hdr + n_bt + q of kmpgpu_set_rules, with or without KMPGPU_RULE_NOT; kmpgpu_scan_rules,
 * kmpgpu_scan_alerts(KMPGPU_ALERT_RULES) and kmpgpu_scan_flows run the regex kernel (one launch) behind the byte-test kernels and in front
 * of the rules kernel.  KMPGPU_FLOW_SCOPE_FLOW folds their rows as it folds every term row; under kmpgpu_scan_flows_seams they stay src's
 * own: no expression is matched across a flow seam.  There is no KMPGPU_ALERT_* family for them: the rules are the route to the alert list,
 * the flows, kmpgpu_load_selected and the export.
 *
 * kmpgpu_scan_regexes: synchronous, on the context's stream.  The marking pass of kmpgpu_scan_packets, then the regex kernel instead of the
 * pattern-level reduce.  Every output may be NULL: rx_pkt_counts_out[n_rx], any_out[W], rx_hits_out[n_rx * W] (layout as
 * kmpgpu_scan_packets), counts_out[n_pat].  Preconditions and errors as kmpgpu_scan_packets; no expressions set: KMPGPU_ESTATE.
 * With no expressions set every output, launch and device buffer of every other call is what it is without these calls.
 * Cost: an expression is a position automaton of at most 63 positions stepped with a handful of 64-bit operations per
 * text byte; its cost is deterministic, its state one 64-bit word, and no memory grows with the payload.  n_rx further rows of the hit
 * matrix, (n_rx x W2 + n_rx) x 8 bytes, and 2080 bytes of table per expression.  The kernel reads every payload's text once per 8
 * expressions, up to the byte at which every expression of the eight is decided.
 *
 * KMPGPU_RX_GROUPS, per expression: the dialect above plus groups and alternation.  ( ... ) and (?: ... ) are groups and
 * mean the same, nothing is captured; | alternates inside a group and at top level; ? * + {n} {n,} {n,m} may stand behind a group, and
 * groups nest, at most 32 deep.  Positions are counted after unrolling: G{n,m} is n copies of G and m - n optional ones, G{n,} n - 1
 * copies and one G+, G* an optional G+.  Refused, in the form above: every other (? form, an empty group or alternative ((a|), (), a||b,
 * |a), a top-level | beside a leading ^ or a trailing $ (write ^(a|b)$: Python reads ^a|b$ as (^a)|(b$)), ^ or $ inside a group, a
 * quantifier on a quantifier ((a)+? too), an unterminated group, a ) without its opening, more than KMPGPU_RX_MAX_POSITIONS positions, and
 * an expression whose automaton needs more than KMPGPU_RX_MAX_EDGES edge rules ("position 0: needs R edge rules, more than 8").  ("position 0: internal: ..." is the compiler's self-check of that
 * derivation; no expression reaches it, kmp_regex.cpp says why.)  The
 * meaning, $, the text end, the gate and the flags are the ones above; an expression with the flag and without ( ) | gives the rows it
 * gives without it.  Without the flag ( ) | stay refused, and bit 8u stays unknown.  A flagged expression costs 2224 bytes of a second
 * table beside its slot of the first.  Launch order wherever the regex kernel runs: the linear kernel if any expression lacks the flag,
 * then the grouped kernel (kmp_regex_groups.hip) if any carries it, both on the context's stream and both recorded by a running profile
 * in front of the rules kernel; a set without a flagged expression launches what it launched. */
#define KMPGPU_RX_NOCASE 1u       /* ASCII case-insensitive */
#define KMPGPU_RX_DOTALL 2u       /* . matches 0x0A too */
#define KMPGPU_RX_GATED  4u       /* only in payloads that hold pattern gate[q] */
#define KMPGPU_RX_GROUPS 16u      /* groups and alternation: the dialect's additions above (bit 8u stays unknown) */
#define KMPGPU_RX_MAX_POSITIONS 63
#define KMPGPU_RX_MAX_EDGES 8     /* edge rules of an expression under KMPGPU_RX_GROUPS */
int  kmpgpu_set_regexes(kmpgpu_ctx *ctx, const uint8_t *const *expr /* [n_rx] */, const uint32_t *expr_len /* [n_rx] */,
                        const uint32_t *flags /* [n_rx]; NULL = all 0 */, const uint32_t *gate /* [n_rx]; NULL = none gated */, uint32_t n_rx);
int  kmpgpu_scan_regexes(kmpgpu_ctx *ctx, uint64_t *rx_pkt_counts_out /* [n_rx] or NULL */, uint64_t *any_out /* [W] or NULL */,
                         uint64_t *rx_hits_out /* [n_rx * W] or NULL */, uint64_t *counts_out /* [n_pat] or NULL: as kmpgpu_scan */,
                         kmpgpu_timing *t /* or NULL */);

/* The alert list: which payloads hit which rows, as records instead of a bit matrix (the hit rows of kmpgpu_scan_packets and the rows of
 * kmpgpu_scan_rules / _relations / _chains are rows x W x 8 bytes that the caller downloads and walks; the answer is normally a handful of
 * (payload, rule) pairs).  The set bits of one row family are compacted on the device into 16-byte records, in capture order.
 * family names the rows, and row[i][k] is exactly the bit the family's own call defines -- under windows, KMPGPU_OPT_WHOLE_PAYLOAD and
 * KMPGPU_PAT_NOCASE, and for rules with relation and chain terms:
 *     KMPGPU_ALERT_PATTERNS   hit[i][k] of kmpgpu_scan_packets,         index = pattern i
 *     KMPGPU_ALERT_RULES      rule_hit[r][k] of kmpgpu_scan_rules,      index = rule r
 *     KMPGPU_ALERT_RELATIONS  rel_hit[q][k] of kmpgpu_scan_relations,   index = relation q
 *     KMPGPU_ALERT_CHAINS     chain_hit[c][k] of kmpgpu_scan_chains,    index = chain c
 * The list is every (packet = k, index = i) with row[i][k] set and k < n_pkts, sorted by packet ascending, then index ascending; no pair
 * appears twice, and the bits of index n_pkts and above never give a record.  The order does not depend on the run: no atomic decides a
 * position.
 *     *n_found        the length of the whole list (it does not depend on max_records)
 *     *n_packets      the distinct payloads in it (may be NULL) = the set bits of the family's any[]
 *     pkt_counts_out  [rows of the family] or NULL: what the family's own call returns under that name (pkt_counts, rule_pkt_counts,
 *                     rel_pkt_counts, chain_pkt_counts)
 *     counts_out      [n_pat] or NULL: exactly what kmpgpu_scan returns
 * Where the records live: the first min(max_records, *n_found) records of the list -- a prefix of the sorted list, not an arbitrary
 * subset; UINT64_MAX: all of them -- are built in a device buffer the context owns, 16 bytes per record, grown like the other buffers
 * and freed by kmpgpu_destroy.  kmpgpu_alerts_read copies records [first, first + n) of that buffer to out (host memory); n == 0 copies
 * nothing (out may be NULL).  A range that leaves the kept prefix: KMPGPU_EINVAL, and the list stays.  No list: KMPGPU_ESTATE -- no
 * kmpgpu_scan_alerts has ended well on the context yet, or since then an arena was loaded, attached, extracted or selected INTO the
 * context (kmpgpu_load_arena, kmpgpu_attach_arena, kmpgpu_load_frames, kmpgpu_load_selected as dst) or patterns were set.  Every
 * kmpgpu_scan_alerts replaces the list, a failed one leaves none.
 * Ordering: synchronous, on the context's stream.  The marking pass of kmpgpu_scan_packets (the same code: zeroing, scan launches), then
 * what the family needs -- the pattern-level reduce, or the relation, chain and rules kernels as kmpgpu_scan_rules orders them --, then the
 * list kernels: count, two scan kernels (the ones kmpgpu_load_frames and kmpgpu_load_selected use, in the scratch kept for them), the
 * totals read once on the host, fill.
 * Preconditions and errors as the family's own call: streaming kernels only (KMPGPU_OPT_MODE 1 or KMPGPU_OPT_KERNEL 1: KMPGPU_EINVAL); an
 * arena kept in place with KMPGPU_OPT_REPACK = 0 is packed once; no patterns, or nothing of the family set: KMPGPU_ESTATE; a context
 * between kmpgpu_load_frames_begin and _finish: KMPGPU_ESTATE; an unknown family or n_found == NULL: KMPGPU_EINVAL; a family of more than
 * 0xFFFFFFFE / 16 = 268 435 455 rows: KMPGPU_EINVAL (a payload's records are scanned as a 32-bit byte length).  With n_pkts == 0
 * everything is 0, nothing is launched and an empty list exists.  When the records cannot be allocated the call fails with KMPGPU_ENOMEM /
 * KMPGPU_EHIP and the context stays usable.
 * What stays as it is: the context's counters (also under KMPGPU_OPT_ACCUMULATE); every output of every other call is bit-identical with
 * and without this call having run; kmpgpu_scan_packets and kmpgpu_scan_rules return the same before and after.
 * *t (may be NULL): kernel_ms from the zeroing to the end of the fill kernel (the host's read of the totals lies inside), d2h_ms the small
 * outputs, launches = the launches of the family's own call + 4 (count, two scan kernels, fill; + 3 where no record is kept and the fill
 * is not launched).  Under kmpgpu_profile_begin the list kernels are recorded last, as three entries: count, the two scan kernels
 * together, fill (where launched); in front of them the family's kernels as its own call records them, and for KMPGPU_ALERT_PATTERNS the
 * pattern-level reduce as one entry.
 * Cost (the figures of tools/alerts.py go to profiles/alerts.txt): the rows are read twice (count and fill), 32 bytes
 * per (row, 256 payloads) and only where any[] has a bit; 20 bytes per payload of scan workspace are written and read; 16 bytes per
 * kept record are written. */
#define KMPGPU_ALERT_PATTERNS  0   /* rows of kmpgpu_scan_packets:   index = pattern  */
#define KMPGPU_ALERT_RULES     1   /* rows of kmpgpu_scan_rules:     index = rule     */
#define KMPGPU_ALERT_RELATIONS 2   /* rows of kmpgpu_scan_relations: index = relation */
#define KMPGPU_ALERT_CHAINS    3   /* rows of kmpgpu_scan_chains:    index = chain    */
typedef struct kmpgpu_alert {
    uint64_t packet;          /* payload index in the arena                                */
    uint32_t index;           /* row of the family: pattern, rule, relation or chain index */
    uint32_t reserved;        /* 0                                                         */
} kmpgpu_alert;
int  kmpgpu_scan_alerts(kmpgpu_ctx *ctx, int family, uint64_t max_records, uint64_t *n_found, uint64_t *n_packets /* or NULL */,
                        uint64_t *pkt_counts_out /* [rows of the family] or NULL */, uint64_t *counts_out /* [n_pat] or NULL: as kmpgpu_scan */,
                        kmpgpu_timing *t /* or NULL */);
int  kmpgpu_alerts_read(kmpgpu_ctx *ctx, kmpgpu_alert *out, uint64_t first, uint64_t n);

/* The payloads a bitmap selects, compacted on the device into a packed arena that a second context owns: the consumer of any[] and of
 * the rows of kmpgpu_scan_packets / kmpgpu_scan_rules (the filter in front of a packet export -- only the selected bytes are downloaded
 * --, and the cascade: a cheap first stage selects, a costly second one -- a thousand patterns, nocase sets -- scans the subset with
 * patterns, rules and windows of its own; its hit rows and offsets refer to the compacted arena, and the bitmap's set bits map them
 * back to the source).
 * Selection: select is W = ceil(n_src / 64) 64-bit words laid out as kmpgpu_scan_packets lays them out (payload k is bit (k & 63) of
 * word (k >> 6)), n_src being src's current payload count; bits of index n_src and above are ignored, whatever they hold.
 * select_on_device == 0: host memory, borrowed for the call and uploaded; == 1: device memory on src's device (8-byte aligned),
 * complete before the call, only read; any other value: KMPGPU_EINVAL.
 * Result: dst owns a packed arena of exactly the selected payloads in ascending source order -- the j-th set bit below n_src is
 * payload j --, each with its source length in a slot of max(16, round_up(len, 16)) bytes, slots back to back from offset 0.  Every
 * byte between a payload's end and its slot's end is 0x00, whatever the source held there (a borrowed source may have dirty padding);
 * an empty payload owns one zero slot.  The arena is in the state kmpgpu_load_frames leaves: owned by the context, padding known
 * clean, packet-start bitmap and plans rebuilt, uniform / packed taken from a device-side pass over the new index, the nocase fold
 * stale (made again by the first pass that needs it).  *n_selected (may be NULL) = the number of payloads.  No payload selected, or
 * n_src == 0 (src without an arena; select may then be NULL): dst is left without an arena, as kmpgpu_load_arena(..., n_pkts = 0)
 * leaves it -- scans return zeros --, the return value is KMPGPU_OK and dst's earlier arena is not kept.
 * Untouched: src is not written; its arena, index and derived state stay, and every output of it is bit-identical before and after.
 * The source is whatever src scans now -- loaded, attached (borrowed), extracted from frames, repacked, or kept in place under
 * KMPGPU_OPT_REPACK = 0 (then not packed: the index is followed as it is).  dst's patterns, flags, rules, windows, options and
 * counters stay too: they belong to the pattern set or the context, not to the arena.
 * Ordering: synchronous.  Waits for dst's stream, as the loaders do, then for src's, as kmpgpu_counts_add does, and works on dst's
 * stream.  dst's owned buffers are reused when the result fits and grown as the loaders grow them otherwise (kmpgpu_reserve sizes
 * them); the workspace is the scratch dst keeps for kmpgpu_load_frames, so a ring of selections does not allocate per call.
 * Errors: dst == src (a context holds one arena), a NULL context, select NULL with n_src > 0, contexts on different devices (no
 * selection across devices): KMPGPU_EINVAL; either context between kmpgpu_load_frames_begin and _finish: KMPGPU_ESTATE; after each of
 * these dst keeps the arena it had.  After an allocation failure (KMPGPU_ENOMEM / KMPGPU_EHIP) dst is without an arena and both
 * contexts stay usable.
 * kmpgpu_last_timing(dst): h2d_ms / h2d_bytes of the bitmap upload (0 for a device bitmap), kernel_ms from the first selection kernel
 * to the copy's end, launches = the kernels in that span (masked lengths, two scan kernels, index, copy: 5; 3 when nothing is selected).
 * Cost: one read of src's lengths and offsets, one read of the selected slots and one write of them. */
int  kmpgpu_load_selected(kmpgpu_ctx *dst, kmpgpu_ctx *src, const void *select /* uint64_t[ceil(n_src / 64)] */, int select_on_device,
                          uint64_t *n_selected /* or NULL */);

/* The payloads of an arena percent-decoded on the device into a packed arena that a second context owns: the normalised buffer the same
 * patterns, rules, byte tests and expressions run over, so that `GET /%61dmin`, `%2e%2e%2f` and `%3Cscript` meet the rules that name
 * `/admin`, `../` and `<script`.  Every other call looks at the payload bytes as they were captured.
 * Definition (transform == KMPGPU_DECODE_PERCENT, the only one; any other value: KMPGPU_EINVAL).  Let payload k of src be the bytes
 * p[0..L), L = pkt_len[k]: the whole payload -- the transform does not look at KMPGPU_OPT_WHOLE_PAYLOAD and does not stop at 0x00.
 *   hex(b): b is one of 0-9 a-f A-F.   esc(i): i + 2 < L and p[i] == '%' and hex(p[i+1]) and hex(p[i+2]).
 * A hex digit is never '%', so escapes cannot overlap, and every position is decided on its own: there is no left-to-right state.
 * The decoded payload is, for i ascending: the byte 16 * val(p[i+1]) + val(p[i+2]) where esc(i); nothing where esc(i-1) or esc(i-2);
 * otherwise p[i] -- under KMPGPU_DECODE_PLUS 0x20 where p[i] == '+' (a '+' that a %2B decodes to stays '+').  So `%%41` gives `%A`,
 * `%2%41` gives `%2A`, and a trailing `%4` or `%` stays.  This is what Python's urllib.parse.unquote_to_bytes computes (with PLUS: after
 * '+' was replaced by ' ').  A %00 yields a 0x00 byte: under dst's default text rule that byte ends the payload's text, which is what a
 * server that takes the decoded bytes as a C string would see; KMPGPU_OPT_WHOLE_PAYLOAD on dst scans behind it.  A byte at or behind L
 * never takes part -- slot padding, whatever a borrowed arena holds there, the next payload: `%4` at a payload's end followed by `1` in
 * dirty padding is not an escape.  changed(k): payload k has at least one escape or, under PLUS, at least one '+' -- the same as "the
 * decoded bytes differ from the original".
 * Result without KMPGPU_DECODE_ONLY_CHANGED: dst owns a packed arena of n_src payloads in source order, payload k the decoding of src's
 * payload k, each in a slot of max(16, round_up(len, 16)) bytes, slots back to back from offset 0.  Every byte between a payload's end
 * and its slot's end is 0x00, whatever the source held there; an empty payload owns one zero slot.  dst's hit rows, any[], alert
 * records and flow ids are in src's numbering.
 * Result with KMPGPU_DECODE_ONLY_CHANGED: dst holds only the payloads with changed(k), compacted in ascending order -- the j-th set bit
 * of the changed bitmap is dst's payload j.  This is the cheap route: scan src raw, scan only the changed payloads decoded, and map back
 * with the bitmap, as the cascade of kmpgpu_load_selected does.  No payload changed, or n_src == 0 (src without an arena): dst is left
 * without an arena, as kmpgpu_load_arena(..., n_pkts = 0) leaves it -- scans return zeros --, the return value is KMPGPU_OK and dst's
 * earlier arena is not kept.
 * Outputs: changed_out (host, may be NULL) takes W = ceil(n_src / 64) words laid out as kmpgpu_scan_packets lays them out (payload k is
 * bit (k & 63) of word (k >> 6)); bits of index n_src and above are 0.  *d_changed (may be NULL) = the same words in a device buffer
 * dst owns, valid until dst's next loader call (NULL where n_src == 0 or the call failed); it is what
 * kmpgpu_load_selected(third, src, ptr, 1, ..) takes, as the d_pkt_bits of kmpgpu_flows_select is.  *stats (may be NULL): n_payloads =
 * the payloads dst holds, n_changed = the set bits of the bitmap, bytes_in = the source bytes of the payloads dst holds, bytes_out =
 * their decoded bytes.
 * State: the metadata goes with the payloads, as in kmpgpu_load_selected, whenever src has some (with ONLY_CHANGED the changed
 * payloads' records in their new order, otherwise a device copy of all of them), so header predicates, kmpgpu_flows_build and
 * flow-scope rules work in dst.  The arena is in the state kmpgpu_load_frames leaves: owned by the context, padding known clean,
 * packet-start bitmap and plans rebuilt, uniform / packed taken from a device-side pass over the new index, the nocase fold stale (made
 * again by the first pass that needs it); flows and seams of dst are dropped.
 * Untouched: src is not written; its arena, index and derived state stay, and every output of it is bit-identical before and after.
 * The source is whatever src scans now -- loaded, attached (borrowed), extracted from frames, selected, decoded, repacked, or kept in
 * place under KMPGPU_OPT_REPACK = 0 (then not packed: the index is followed as it is).  A decoded arena can be decoded again: `%252e`
 * takes two calls, through a third context or back and forth between two.  dst's patterns, flags, rules, windows, options and counters
 * stay: they belong to the pattern set or the context, not to the arena.
 * Ordering: synchronous.  Waits for dst's stream, as the loaders do, then for src's, and works on dst's stream.  dst's owned buffers
 * are reused when the result fits and grown as the loaders grow them otherwise (an eighth of headroom; kmpgpu_reserve sizes them); the
 * workspace is the scratch dst keeps for kmpgpu_load_frames, and the bitmap's buffer is kept too, so a ring of calls does not allocate
 * per call.
 * Errors: dst == src (a context holds one arena), a NULL context, contexts on different devices (no decoding across devices), an
 * unknown transform, an unknown flag bit: KMPGPU_EINVAL; either context between kmpgpu_load_frames_begin and _finish: KMPGPU_ESTATE;
 * after each of these dst keeps the arena it had.  After an allocation failure (KMPGPU_ENOMEM / KMPGPU_EHIP) dst is without an arena
 * and both contexts stay usable.
 * kmpgpu_last_timing(dst): kernel_ms from the first decode kernel to the write's end, launches = the kernels in that span (decoded
 * lengths, two scan kernels, index, write: 5; 3 where dst ends up without a payload); the metadata's copy or kernel follows the span.
 * kmpgpu_profile_begin .. _end time the span in four pairs: lengths, scan, index, write.
 * Cost: two reads of src's payload bytes (lengths, write) and one write of the decoded ones. */
#define KMPGPU_DECODE_PERCENT      1      /* transform */
#define KMPGPU_DECODE_PLUS         1u     /* flags: '+' decodes to 0x20 */
#define KMPGPU_DECODE_ONLY_CHANGED 2u     /* dst holds the changed payloads only */
typedef struct kmpgpu_decode_stats { uint64_t n_payloads, n_changed, bytes_in, bytes_out; } kmpgpu_decode_stats;
int  kmpgpu_load_decoded(kmpgpu_ctx *dst, kmpgpu_ctx *src, int transform, uint32_t flags,
                         uint64_t *changed_out /* host [ceil(n_src / 64)] or NULL */, const void **d_changed /* or NULL */,
                         kmpgpu_decode_stats *stats /* or NULL */);

/* The base64 runs of an arena's payloads decoded on the device into a packed arena that a second context owns, so that
 * `Authorization: Basic YWRtaW46YWRtaW4=`, a JWT in a cookie, `powershell -enc ...` or a base64 blob in a body meet the rules that
 * name what the base64 holds (`admin:admin`).  A sibling of kmpgpu_load_decoded: a call of its own, not a value of `transform`.
 * Definition.  Let payload k of src be the bytes p[0..L), L = pkt_len[k]: the whole payload -- the call does not look at
 * KMPGPU_OPT_WHOLE_PAYLOAD and does not stop at 0x00.  No byte at or behind L takes part: slot padding, a borrowed arena's dirty
 * padding, the next slot.
 *   alpha(b): b is one of A-Z a-z 0-9 + /; under KMPGPU_B64_URLSAFE the last two are - and _ instead, and + and / are then not
 *     alphabet.  val(b) is 0..63 in that order.
 *   Run: a maximal interval [s, e) of alphabet bytes inside the payload: s == 0 or !alpha(p[s-1]), and e == L or !alpha(p[e]).  Its
 *     length is m = e - s.
 *   Decoded run: a run with m >= min_run, 4 <= min_run <= 255.
 *   A decoded run yields floor(3m / 4) bytes: the alphabet byte at run offset r = i - s yields nothing where r % 4 == 0, otherwise the
 *     byte ((val(p[i-1]) << 2 * (r % 4)) | (val(p[i]) >> (6 - 2 * (r % 4)))) & 0xFF.  Leftover bits at the run's end are dropped,
 *     whatever they are: 6 bits for m % 4 == 1, then 4 and 2.
 *   Padding: directly behind a decoded run with m % 4 == 2 the first up to two '=' yield nothing, with m % 4 == 3 the first one; they
 *     must lie inside the payload.
 *   Every other byte is copied: alphabet bytes of shorter runs, other '=', everything else.
 *   changed(k): payload k holds at least one decoded run -- the same as "the output differs from the payload", because a decoded run
 *     always shrinks.
 * This is Python's base64 module run by run: re.sub over ([alphabet]{min_run,})(={0,2}), the run (less its last character where
 * m % 4 == 1) padded to a multiple of 4 and given to b64decode / urlsafe_b64decode, the '=' that the padding rule does not consume put
 * back.  A decoded 0x00 ends the payload's text under dst's default text rule, as %00 does.
 * min_run is the caller's guard against decoding ordinary words: every run of that many letters and digits IS base64 by this
 * definition.  `Authorization: Basic YWRtaW46YWRtaW4=\r\n` at min_run = 14 becomes `Authorization: Basic admin:admin\r\n`; at
 * min_run = 8 the word `Authorization` (13 letters) is itself a decoded run and comes out as 9 bytes of noise.  That is the definition
 * and not a defect: the raw context still holds the word, and the caller combines rows of contexts that share src's numbering, as for
 * the percent-decoded buffer.  Choose min_run above the longest word the rules on dst must still see and at or below the shortest
 * encoded value they look for (16 covers a 12-byte secret).
 * Result, outputs (changed_out, *d_changed, *stats), state, ordering, buffers, KMPGPU_B64_ONLY_CHANGED and the empty cases (no payload
 * changed, n_src == 0: dst left without an arena, KMPGPU_OK) are those of kmpgpu_load_decoded, word for word: slots of
 * max(16, round_up(len, 16)) bytes back to back from offset 0, every slot's tail 0x00 whatever the source held, an empty result payload
 * owning one zero slot; the metadata goes along; dst's rows are in src's numbering, or numbered through the changed bitmap; *d_changed
 * is what kmpgpu_load_selected takes.  The source is whatever src scans now, a decoded, field, stream or base64 arena included: a
 * twice-encoded value takes two calls.
 * Errors: a NULL context, dst == src, min_run outside 4..255, an unknown flag bit, contexts on different devices: KMPGPU_EINVAL;
 * either context between kmpgpu_load_frames_begin and _finish: KMPGPU_ESTATE.  After each of these dst keeps the arena it had, *stats
 * is zero and *d_changed NULL.  Allocation failures: as kmpgpu_load_decoded.
 * kmpgpu_last_timing(dst): kernel_ms from the lengths kernel to the write's end, launches = the kernels in that span (base64 lengths,
 * two scan kernels, index, write: 5; 3 where dst ends up without a payload); the metadata's copy or kernel follows the span.
 * kmpgpu_profile_begin .. _end time the span in four pairs: lengths, scan, index, write.
 * Cost: two reads of src's payload bytes (lengths, write) and one write of the decoded ones. */
#define KMPGPU_B64_URLSAFE      1u     /* flags: the alphabet ends in - _ instead of + / */
#define KMPGPU_B64_ONLY_CHANGED 2u     /* dst holds the changed payloads only */
int  kmpgpu_load_base64(kmpgpu_ctx *dst, kmpgpu_ctx *src, uint32_t min_run, uint32_t flags,
                        uint64_t *changed_out /* host [ceil(n_src / 64)] or NULL */, const void **d_changed /* or NULL */,
                        kmpgpu_decode_stats *stats /* or NULL */);

/* HTTP field buffers: the method, the URI, the status, the headers or the body of the HTTP message at the start of every payload, as a
 * packed arena that a second context owns -- the sticky buffers of signature languages (http_method, http_raw_uri, http_stat_code,
 * http_header, http_client_body).  That context scans it with everything the library has, in src's payload numbering, so a rule that
 * names `/admin` meets the request line only, not a Referer: header or a body.  kmpgpu_load_decoded over the RAW_URI context gives the
 * normalised URI.  Every other call looks at a payload as one undivided byte string.
 * Definition.  Let payload k be the bytes p[0..L), L = pkt_len[k]: the whole payload -- the locate does not look at
 * KMPGPU_OPT_WHOLE_PAYLOAD and does not stop at 0x00.  No byte at or behind L takes part: slot padding of a borrowed arena, the next slot
 * and the arena's end are all excluded.  Every term is "the smallest index with a local property"; there is no left-to-right state.
 *   Start line end.  e = the smallest i with p[i] == '\n', or L if there is none.  e' = e - 1 if e >= 1 and p[e-1] == '\r', otherwise
 *     e' = e.  The start line is p[0..e').
 *   Tokens.  s1 = the smallest i < e' with p[i] == ' '.  s2 = the smallest i with s1 < i < e' and p[i] == ' ', or e' if there is none.
 *   kind.  RESPONSE if e' >= 5 and p[0..5) == "HTTP/".  Otherwise REQUEST if s1 exists, 1 <= s1 <= 15, every byte of p[0..s1) is in
 *     A..Z, and s1 + 1 < e'.  Otherwise NONE, and every field is absent.  (The bound 15 is deliberate: a payload is ruled out from its
 *     first 16-byte unit alone.)
 *   METHOD (REQUEST): p[0..s1).
 *   RAW_URI (REQUEST): p[s1+1..s2).  It may be empty.
 *   STATUS (RESPONSE, present iff s1 exists and s1 + 1 < e'): p[s1+1..s2).
 *   HEADERS (both kinds, present iff e < L).  bl = the smallest i >= e with p[i] == '\n' and one of: i + 1 < L and p[i+1] == '\n'; or
 *     i + 2 < L and p[i+1] == '\r' and p[i+2] == '\n'.  HEADERS is p[e+1..h1) with h1 = bl + 1, or h1 = L where there is no bl (the
 *     segment cut the headers).  bl == e gives empty headers, which are still present.
 *   BODY (present iff bl exists): p[b0..L), b0 = bl + 2 or bl + 3 according to which form matched.  It may be empty.
 * A present field of length 0 and an absent field both become an empty payload of dst (one zero slot); the present bitmap tells them
 * apart.  Limits: one message per payload, the one at its start; no chunked or compressed bodies, no header folding, no
 * per-header buffers; methods are 1 to 15 upper-case letters.  A rule over several buffers takes the other buffers' rows
 * through links (kmpgpu_link_rows).
 *
 * kmpgpu_http_locate decides all of this for every payload of ctx's arena in one kernel and keeps one kmpgpu_http_span per payload on
 * the device.  Offsets count from the payload's first byte; an absent field has offset and length 0; a NONE payload's record is all
 * zero.  tok_off / tok_len are RAW_URI for a request and STATUS for a response (KMPGPU_HTTP_HAS_TOKEN: it is present), METHOD is
 * p[0..method_len).  *stats (may be NULL): the requests, the responses, the messages (not NONE) with a blank line, and bytes_scanned, the
 * payload bytes the kernel looked at: min(L, 16) for a payload that its first 16 bytes rule out, otherwise min(L, 1024 (t + 1)) where
 * step t = i / 1024 ends the search -- i = bl; or i = e where the start line makes the payload NONE after all; or i = L - 1.  The spans belong to the arena: every call that changes it drops them (the calls that drop the flows),
 * a scan does not; with valid spans the call launches nothing and hands out the stats again.  kmpgpu_http_spans_read copies records
 * [first, first + n) to the host (KMPGPU_ESTATE without valid spans, KMPGPU_EINVAL for a range that leaves them).  Both are synchronous
 * on ctx's stream; KMPGPU_ESTATE between kmpgpu_load_frames_begin and _finish.  kmpgpu_last_timing: kernel_ms of the locate, launches
 * = 1 (0 where the spans were valid); kmpgpu_profile_begin .. _end time it as one pair.
 *
 * kmpgpu_load_fields makes dst's arena the field `field` of every payload of src.  It runs the locate on src first where src's spans
 * are stale (that cache is all of src that is written: its arena, index and derived state stay, and every output of it is bit-identical
 * before and after); a ring of calls for several fields pays it once.
 * Result without KMPGPU_FIELDS_ONLY_PRESENT: dst owns a packed arena of n_src payloads in source order, payload k the field of src's
 * payload k (empty where absent), each in a slot of max(16, round_up(len, 16)) bytes, slots back to back from offset 0, every byte
 * between a payload's end and its slot's end 0x00.  With it: only the payloads whose field is present, compacted in ascending order --
 * the j-th set bit of the present bitmap is dst's payload j.  No payload held, or n_src == 0: dst is left without an arena, the return
 * value is KMPGPU_OK and dst's earlier arena is not kept.
 * Outputs, state, ordering and buffers are those of kmpgpu_load_decoded, word for word: present_out / *d_present as changed_out /
 * *d_changed (the device words are what kmpgpu_load_selected(third, src, ptr, 1, ..) takes; they share the buffer of *d_changed, valid
 * until dst's next loader call); *stats: n_payloads = the payloads dst holds, n_present = the set bits, bytes_in = the source bytes of
 * the payloads dst holds, bytes_out = their field bytes.  The metadata goes with the payloads (a device copy, or the present payloads'
 * records in their new order), so header predicates, kmpgpu_flows_build and flow-scope rules work in dst and give src's flow ids.  The
 * arena is in the state kmpgpu_load_frames leaves: owned, padding clean, bitmap and plans rebuilt, the fold stale, flows, seams and
 * spans of dst dropped.  Synchronous on dst's stream after waiting for src's; the workspace is the scratch dst keeps for
 * kmpgpu_load_frames, so a ring of calls does not allocate per call.  The source is whatever src scans now: loaded, attached with dirty
 * padding, extracted, selected, decoded, streams, or kept in place under KMPGPU_OPT_REPACK = 0.
 * Errors, all refused before any launch: dst == src, a NULL context, contexts on different devices, an unknown field, an unknown flag
 * bit: KMPGPU_EINVAL; either context between kmpgpu_load_frames_begin and _finish: KMPGPU_ESTATE; after each of these dst keeps the
 * arena it had.  After an allocation failure dst is without an arena and both contexts stay usable.
 * kmpgpu_last_timing(dst): kernel_ms from the first kernel to the gather's end, launches = the kernels in that span (field lengths, two
 * scan kernels, index, gather: 5; 3 where dst ends up without a payload; one more where the locate ran).  kmpgpu_profile_begin .. _end
 * time the span as the locate's pair (where it ran), then four pairs: lengths, scan, index, gather.
 * Cost: the locate reads the first 16 bytes of every payload and of the messages what lies in front of their blank
 * line in steps of 1 KiB; the load reads the spans twice and the field bytes once and writes them once. */
#define KMPGPU_HTTP_NONE      0      /* kmpgpu_http_span.kind */
#define KMPGPU_HTTP_REQUEST   1
#define KMPGPU_HTTP_RESPONSE  2
#define KMPGPU_HTTP_HAS_LF    1u     /* kmpgpu_http_span.flags: e < L (HEADERS present) */
#define KMPGPU_HTTP_HAS_BLANK 2u     /* bl exists (BODY present) */
#define KMPGPU_HTTP_HAS_TOKEN 4u     /* tok_off / tok_len are a present field: RAW_URI of a request, STATUS of a response */
typedef struct kmpgpu_http_span {
    uint8_t  kind, flags;
    uint16_t method_len;
    uint32_t tok_off, tok_len, hdr_off, hdr_len, body_off, body_len, reserved;
} kmpgpu_http_span;
typedef struct kmpgpu_http_stats { uint64_t n_requests, n_responses, n_blank, bytes_scanned; } kmpgpu_http_stats;
int  kmpgpu_http_locate(kmpgpu_ctx *ctx, kmpgpu_http_stats *stats /* or NULL */);
int  kmpgpu_http_spans_read(kmpgpu_ctx *ctx, kmpgpu_http_span *out, uint64_t first, uint64_t n);
#define KMPGPU_FIELD_METHOD   1
#define KMPGPU_FIELD_RAW_URI  2
#define KMPGPU_FIELD_STATUS   3
#define KMPGPU_FIELD_HEADERS  4
#define KMPGPU_FIELD_BODY     5
#define KMPGPU_FIELDS_ONLY_PRESENT 1u     /* flags: dst holds only the payloads whose field is present */
typedef struct kmpgpu_fields_stats { uint64_t n_payloads, n_present, bytes_in, bytes_out; } kmpgpu_fields_stats;
int  kmpgpu_load_fields(kmpgpu_ctx *dst, kmpgpu_ctx *src, int field, uint32_t flags,
                        uint64_t *present_out /* host [ceil(n_src / 64)] or NULL */, const void **d_present /* or NULL */,
                        kmpgpu_fields_stats *stats /* or NULL */);

/* DNS query-name buffers: the name of the first question of the DNS message in every payload, in dotted form, as a packed arena that a
 * second context owns -- the dns.query / dns_query buffer of signature languages.  On the wire `www.youtube.com` is
 * \x03www\x07youtube\x03com\x00, so no pattern over the payload itself can name a host; in dst a pattern `youtube.com` can.
 * Definition.  Let payload k be the bytes p[0..L), L = pkt_len[k]: the whole payload, whatever KMPGPU_OPT_WHOLE_PAYLOAD says.  No byte at
 * or behind L takes part: slot padding of a borrowed arena may be dirty.  b = 2 under KMPGPU_DNS_TCP_PREFIX (DNS over TCP: a 2-byte
 * length in front, which is not checked against L), otherwise b = 0.  Let m[i] = p[b + i] and M = L - b.
 * The payload is NONE, with every field absent and an all-zero record, unless all of these hold:
 *   M >= 17.
 *   QDCOUNT = be16(m[4..6)) >= 1.
 *   The walk succeeds.  It starts at i_0 = 12.  At step t, c = m[i_t] needs i_t < M.  c == 0 ends the name at i_end = i_t.  1 <= c <= 63
 *     needs i_t + 1 + c <= M and gives i_{t+1} = i_t + 1 + c.  c >= 64 makes the payload NONE: a compression pointer or a reserved label
 *     type (a pointer in the first question can only point into the header).
 *   i_end + 1 - 12 <= 255: the wire length of a name, so at most 127 labels.
 *   i_end + 5 <= M: QTYPE and QCLASS lie inside the payload.
 * Fields of a payload that is not NONE:
 *   kind is QUERY where bit 15 of the flags word be16(m[2..4)) is clear, otherwise RESPONSE.
 *   QNAME is the bytes m[13..i_end) with every m[i_t], t >= 1, replaced by '.'.  It is always present, and its length is
 *     max(0, i_end - 13).  The root name is present and empty.
 *   Bytes are taken as they are: no escaping of a '.' or a control byte inside a label, and no case folding -- nocase patterns are the
 *     route against 0x20 mixing.
 * Limits: the first question's name only; no compression pointers; no names of answers, authorities or RDATA; no
 * detection by port; one message per payload; no IDNA decoding.
 *
 * kmpgpu_dns_locate decides all of this for every payload of ctx's arena in one kernel and keeps one kmpgpu_dns_span per payload on the
 * device.  Offsets count from p[0]: name_off = b + 13, q_end = b + i_end + 5; id, qtype, qclass and the four counts are host-order values
 * of the big-endian wire fields, n_labels the labels walked; a NONE payload's record is all zero.  flags: 0 or KMPGPU_DNS_TCP_PREFIX.
 * *stats (may be NULL): the queries, the responses, the root names among both, and the bytes of all names.  The spans belong to the
 * arena: exactly the calls that drop the HTTP spans drop them, a scan does not.  They are valid for the prefix flag they were made with:
 * with valid spans of the same flag the call launches nothing and hands out the stats again, with the other flag it runs again.
 * kmpgpu_dns_spans_read copies records [first, first + n) to the host (KMPGPU_ESTATE without valid spans, KMPGPU_EINVAL for a range that
 * leaves them).  Both are synchronous on ctx's stream; KMPGPU_ESTATE between kmpgpu_load_frames_begin and _finish, KMPGPU_EINVAL for an
 * unknown flag bit.  kmpgpu_last_timing: kernel_ms of the locate, launches = 1 (0 where the spans were valid); kmpgpu_profile_begin ..
 * _end time it as one pair.
 *
 * kmpgpu_load_dns makes dst's arena the field `field` (KMPGPU_DNS_QNAME) of every payload of src, running the locate on src first where
 * src's spans are stale or of the other prefix flag.  flags: KMPGPU_DNS_ONLY_PRESENT (dst holds only the payloads that are messages) and
 * KMPGPU_DNS_TCP_PREFIX.  The result layout, present_out / *d_present, *stats, the metadata carried along, the state dst's arena is left
 * in, dst without an arena and KMPGPU_OK where no payload is held or n_src == 0, the workspace and the ordering are those of
 * kmpgpu_load_fields, word for word; src keeps everything but its span cache, and every output of it is bit-identical before and after.
 * Errors, all refused before any launch: dst == src, a NULL context, contexts on different devices, an unknown field, an unknown flag
 * bit: KMPGPU_EINVAL; either context between kmpgpu_load_frames_begin and _finish: KMPGPU_ESTATE; after each of these dst keeps the
 * arena it had.  kmpgpu_last_timing(dst) and kmpgpu_profile_begin .. _end: as kmpgpu_load_fields (lengths, two scan kernels, index,
 * gather: 5 launches; 3 where dst ends up without a payload; one more where the locate ran).
 * Cost: the locate reads the first 16 bytes of every payload and of the messages the units that hold a length byte
 * of the name; the load reads the spans twice, the separator masks and the name bytes once, and writes the names once. */
#define KMPGPU_DNS_NONE      0      /* kmpgpu_dns_span.kind */
#define KMPGPU_DNS_QUERY     1
#define KMPGPU_DNS_RESPONSE  2
typedef struct kmpgpu_dns_span {
    uint8_t  kind, n_labels;
    uint16_t flags;                    /* the flags word */
    uint16_t id, qtype, qclass, qdcount, ancount, nscount, arcount, reserved;
    uint32_t name_off, name_len, q_end;
} kmpgpu_dns_span;
typedef struct kmpgpu_dns_stats { uint64_t n_queries, n_responses, n_root, name_bytes; } kmpgpu_dns_stats;
#define KMPGPU_DNS_QNAME        1      /* field */
#define KMPGPU_DNS_ONLY_PRESENT 1u     /* flags of kmpgpu_load_dns: dst holds only the payloads that are DNS messages */
#define KMPGPU_DNS_TCP_PREFIX   2u     /* flags of both: a 2-byte length stands in front of the message */
int  kmpgpu_dns_locate(kmpgpu_ctx *ctx, uint32_t flags, kmpgpu_dns_stats *stats /* or NULL */);
int  kmpgpu_dns_spans_read(kmpgpu_ctx *ctx, kmpgpu_dns_span *out, uint64_t first, uint64_t n);
int  kmpgpu_load_dns(kmpgpu_ctx *dst, kmpgpu_ctx *src, int field, uint32_t flags,
                     uint64_t *present_out /* host [ceil(n_src / 64)] or NULL */, const void **d_present /* or NULL */,
                     kmpgpu_fields_stats *stats /* or NULL */);

/* TLS ClientHello buffers: the server name (SNI) and the ALPN protocol list of the ClientHello in every payload, each as a packed arena
 * that a second context owns -- the tls.sni / tls_sni buffer of signature languages, and the ALPN list as `h2,http/1.1`.  They are the
 * only text of a TLS connection a signature can name; a pattern over the payload cannot tell the server name from the same bytes
 * anywhere else, and the ALPN names are length-prefixed on the wire as DNS labels are.
 * Definition.  Let payload k be the bytes p[0..L), L = pkt_len[k]: the whole payload, whatever KMPGPU_OPT_WHOLE_PAYLOAD says.  No byte at
 * or behind L takes part: slot padding of a borrowed arena may be dirty.  be16 and be24 are big-endian reads.
 * The payload is NONE, with every field absent and an all-zero record, unless all of these hold:
 *   The fixed header.  L >= 11, p[0] == 22 (handshake), p[1] == 3, p[2] <= 4, p[5] == 1 (client_hello), p[9] == 3; with rec = be16(p + 3)
 *     and hs = be24(p + 6): rec >= hs + 4, the hello lies in one record.  All of this sits in the first aligned 16-byte unit.
 *   The fixed part.  Let H = 9 + hs and E = min(L, H).  43 < E and sid = p[43] <= 32.  c = 44 + sid needs c + 2 <= E; cs = be16(p + c)
 *     is even and >= 2.  c += 2 + cs needs c < E; cm = p[c] >= 1.  c += 1 + cm.  c == H: the hello has no extensions, it is valid and
 *     both fields are absent.  Otherwise c + 2 <= E, X = c + 2 + be16(p + c) == H, and c += 2.  Let Xe = min(X, E): the hello is
 *     TRUNCATED where Xe < X.
 *   The extension walk.  While c + 4 <= Xe: t = be16(p + c), n = be16(p + c + 2), b = c + 4.  b + n > X makes the payload NONE.
 *     b + n > Xe ends the walk (only in a truncated hello).  Otherwise the extension counts, and a 256th makes the payload NONE; the
 *     first with t == 0 is the server name, the first with t == 16 is ALPN, any other and every later one of these two is stepped over
 *     unread; c = b + n.  A hello that is not truncated ends the walk with c == X.
 *   The server name.  n >= 5; ll = be16(p + b) with ll + 2 <= n; p[b + 2] == 0 (host_name); nl = be16(p + b + 3) with 3 + nl <= ll.  Any
 *     other shape makes the payload NONE.
 *   ALPN.  n >= 4; ll = be16(p + b) with ll + 2 == n and ll >= 2; any other shape makes the payload NONE.  ll > 256 makes ALPN absent and
 *     sets ALPN_SKIPPED (the separator mask is 256 bits wide).  Otherwise, from b + 2 on, every name has a length byte 1 .. 255 and the
 *     names end exactly at b + 2 + ll; any other shape makes the payload NONE.
 * Fields of a payload that is not NONE:
 *   SNI is the bytes p[b + 5 .. b + 5 + nl) as they are: the first entry only, no case folding, no IDNA.  nl == 0 is present and empty.
 *   ALPN is the bytes p[b + 3 .. b + 2 + ll) with every later length byte replaced by ',': h2,http/1.1.
 *   A truncated hello keeps whatever fields its whole extensions gave it.
 * Limits: one hello per payload, at its start; no hello split over records, no SSLv2 hello; no DTLS, no QUIC; no
 * encrypted client hello; no second server_name entry; no JA3 / JA4; no detection by port; no ServerHello, no certificates.  A hello
 * split over TCP segments is found whole only through a stream context (kmpgpu_load_streams).
 *
 * kmpgpu_tls_locate decides all of this for every payload of ctx's arena in one kernel and keeps one kmpgpu_tls_span per payload on the
 * device.  Offsets count from p[0]; record_version = be16(p + 1), client_version = be16(p + 9), hs_len = hs, sid_len = sid, n_suites =
 * cs / 2, n_ext the extensions that counted, n_alpn the names walked; an absent field has offset and length 0; a NONE payload's record
 * is all zero.  flags: 0.  *stats (may be NULL): the hellos, those with a server name, those with an ALPN field, the truncated ones.  The
 * spans belong to the arena: exactly the calls that drop the HTTP and DNS spans drop them, a scan does not.  With valid spans the call
 * launches nothing and hands out the stats again.  kmpgpu_tls_spans_read copies records [first, first + n) to the host (KMPGPU_ESTATE
 * without valid spans, KMPGPU_EINVAL for a range that leaves them).  Both are synchronous on ctx's stream; KMPGPU_ESTATE between
 * kmpgpu_load_frames_begin and _finish, KMPGPU_EINVAL for an unknown flag bit.  kmpgpu_last_timing: kernel_ms of the locate, launches =
 * 1 (0 where the spans were valid); kmpgpu_profile_begin .. _end time it as one pair.
 *
 * kmpgpu_load_tls makes dst's arena the field `field` (KMPGPU_TLS_SNI or KMPGPU_TLS_ALPN) of every payload of src, running the locate
 * on src first where src's spans are stale.  flags: KMPGPU_TLS_ONLY_PRESENT (dst holds only the payloads whose field is present, as
 * kmpgpu_load_fields; without it a payload without the field is an empty payload, in src's numbering).  The result layout, present_out
 * / *d_present, *stats, the metadata carried along, the state dst's arena is left in, dst without an arena and KMPGPU_OK where no
 * payload is held or n_src == 0, the workspace and the ordering are those of kmpgpu_load_fields, word for word; src keeps everything
 * but its span cache, and every output of it is bit-identical before and after.  Errors, all refused before any launch: dst == src, a
 * NULL context, contexts on different devices, an unknown field, an unknown flag bit: KMPGPU_EINVAL; either context between
 * kmpgpu_load_frames_begin and _finish: KMPGPU_ESTATE; after each of these dst keeps the arena it had.  kmpgpu_last_timing(dst) and
 * kmpgpu_profile_begin .. _end: as kmpgpu_load_fields (5 launches; 3 where dst ends up without a payload; one more where the locate ran).
 * A TLS buffer links like any other context: kmpgpu_link_rows with the identity map, or the present bitmap under ONLY_PRESENT.
 * Cost: the locate reads the first 16 bytes of every payload and of the hellos the units that hold a length field of
 * the walk; the load reads the spans twice, for ALPN the separator masks, the field's bytes once, and writes the field once. */
#define KMPGPU_TLS_NONE          0      /* kmpgpu_tls_span.kind */
#define KMPGPU_TLS_CLIENT_HELLO  1
#define KMPGPU_TLS_HAS_SNI       1u     /* kmpgpu_tls_span.flags */
#define KMPGPU_TLS_HAS_ALPN      2u
#define KMPGPU_TLS_TRUNCATED     4u
#define KMPGPU_TLS_ALPN_SKIPPED  8u
typedef struct kmpgpu_tls_span {
    uint8_t  kind, flags, n_ext, sid_len;
    uint16_t record_version, client_version, n_suites, n_alpn;
    uint32_t hs_len, sni_off, sni_len, alpn_off, alpn_len;
} kmpgpu_tls_span;
typedef struct kmpgpu_tls_stats { uint64_t n_hellos, n_sni, n_alpn, n_truncated; } kmpgpu_tls_stats;
#define KMPGPU_TLS_SNI          1      /* field */
#define KMPGPU_TLS_ALPN         2
#define KMPGPU_TLS_ONLY_PRESENT 1u     /* flags of kmpgpu_load_tls: dst holds only the payloads that have the field */
int  kmpgpu_tls_locate(kmpgpu_ctx *ctx, uint32_t flags /* 0 */, kmpgpu_tls_stats *stats /* or NULL */);
int  kmpgpu_tls_spans_read(kmpgpu_ctx *ctx, kmpgpu_tls_span *out, uint64_t first, uint64_t n);
int  kmpgpu_load_tls(kmpgpu_ctx *dst, kmpgpu_ctx *src, int field, uint32_t flags,
                     uint64_t *present_out /* host [ceil(n_src / 64)] or NULL */, const void **d_present /* or NULL */,
                     kmpgpu_fields_stats *stats /* or NULL */);

/* Flows: the payloads of the arena grouped by the 5-tuple of their metadata (kmpgpu_pkt_meta, above), on the device -- which payloads
 * belong to one connection, what each connection carried, and the hit rows of every family folded from payload space into flow space.
 * Definitions.  With M = meta[k], the two endpoints of payload k are the 48-bit integers e_src = src_ip << 16 | src_port and
 * e_dst = dst_ip << 16 | dst_port.
 *     key(k) = (M.proto, min(e_src, e_dst), max(e_src, e_dst))      the default: both directions of a conversation are one flow
 *     key(k) = (M.proto, e_src, e_dst)                              under KMPGPU_FLOW_DIRECTED
 * `reserved` is not part of the key.  A:1 -> B:2 and A:2 -> B:1 are different flows either way.  The protocol byte is part of the key (the
 * UDP frames the tcp extractor accepts do not merge with TCP ones).  Two payloads are in one flow iff their keys are equal.  Flows are
 * numbered 0 .. n_flows - 1 in the order of their first payload; flow_of[k] is payload k's flow.  Neither the numbering nor any output
 * depends on the run: no atomic decides an id.
 * kmpgpu_flows_build groups the arena's payloads (*n_flows, may be NULL) and keeps flow_of[n_pkts] and the records kmpgpu_flow[n_flows] on
 * the device; kmpgpu_flows_read copies records [first, first + n) to out, kmpgpu_flow_ids_read flow_of[first .. first + n).  n == 0
 * copies nothing (out may be NULL).  A record: first_packet / last_packet are the flow's lowest and highest payload index, n_packets its
 * payloads, payload_bytes the sum of their L_k (the index's lengths, whatever KMPGPU_OPT_WHOLE_PAYLOAD says), first = meta[first_packet] as
 * it is (its direction is the flow's).
 *
 * kmpgpu_scan_flows: a flow-space hit matrix beside the payload-space one.  Wf = ceil(n_flows / 64); the layout is that of
 * kmpgpu_scan_packets with flows in place of payloads (flow f is bit (f & 63) of word (f >> 6)); bits at n_flows and above are 0 in every
 * word.  family is one of KMPGPU_ALERT_*.
 *   KMPGPU_FLOW_SCOPE_PACKET (any family): flow_hit[r][f] = OR over the payloads k of flow f of row[r][k], where row is exactly the bit
 *     the family's own call defines (windows, nocase, whole payloads; for rules the relation, chain, header and byte-test terms): the flow holds a
 *     payload that the row matches.
 *   KMPGPU_FLOW_SCOPE_FLOW (KMPGPU_ALERT_RULES only; any other family: KMPGPU_EINVAL): every term row -- patterns, relations, chains, header
 *     predicates, byte tests, as the rule terms index them -- is folded first, then the rule is evaluated per flow:
 *       flow_rule_hit[r][f] = AND over positive terms t of (OR_k row[t][k]) AND AND over negated terms t of !(OR_k row[t][k])
 *     the cross-packet signature: one content in one payload, another in another payload of the same connection.  An all-negated rule
 *     matches every flow that holds none of its terms.
 *   flow_counts[r] = the flows in row r, any[f] = OR over the rows, counts = what kmpgpu_scan returns.  Every output may be NULL.
 * Ordering: synchronous, on the context's stream.  The marking pass and the family's kernels as the family's own call runs them (for
 * SCOPE_FLOW: as kmpgpu_scan_rules), then the fold kernel, then for SCOPE_PACKET the reduce of kmpgpu_scan_packets over the folded matrix,
 * for SCOPE_FLOW the rules kernel of kmpgpu_scan_rules over the folded term rows with n_flows in place of n_pkts.  *t: as the family's own
 * call, launches = its launches + 2 (fold; reduce or rules).  Under kmpgpu_profile_begin those two are recorded last, behind the family's
 * kernels as kmpgpu_scan_alerts records them.
 *
 * kmpgpu_flows_select expands a flow bitmap (uint64_t[Wf]; on_device == 0: host memory, == 1: device memory, 8-byte aligned, complete
 * before the call; bits of index n_flows and above are ignored) to the payload bitmap pkt[k] = flow_bits[flow_of[k]], W = ceil(n_pkts / 64)
 * words, to pkt_bits_out (host, may be NULL) and into a device buffer the context owns (*d_pkt_bits, may be NULL), which stays valid until
 * the next kmpgpu_flows_select on the context or until the flows are dropped.  It is what kmpgpu_load_selected(dst, ctx, ptr, 1, ..)
 * takes: any[] of kmpgpu_scan_flows goes in, the whole connections that fired come out as an arena, with their metadata.  One kernel: a
 * lane per payload, a ballot per word, 8-byte stores.
 *
 * State.  Flows belong to the arena and its metadata: whatever replaces or releases the arena (kmpgpu_load_arena, kmpgpu_attach_arena,
 * kmpgpu_load_frames, kmpgpu_load_selected as dst) and kmpgpu_set_meta drop them (the buffers stay for the next build).  They survive
 * the on-device repack, kmpgpu_set_patterns, the setters of the row families and every option.
 * Errors.  kmpgpu_flows_build: no metadata: KMPGPU_ESTATE ("no packet metadata"); between kmpgpu_load_frames_begin and _finish:
 * KMPGPU_ESTATE; an unknown flag bit: KMPGPU_EINVAL; n_pkts > 2^32 - 2: KMPGPU_EINVAL (ids are 32 bits); KMPGPU_OPT_FLOW_SLOTS neither 0 nor
 * a power of two > n_pkts: KMPGPU_EINVAL.  With n_pkts == 0 it leaves 0 flows and launches nothing.  The read calls, kmpgpu_scan_flows and
 * kmpgpu_flows_select without built flows: KMPGPU_ESTATE; a read range that leaves [0, n_flows) ([0, n_pkts) for the ids): KMPGPU_EINVAL.
 * kmpgpu_scan_flows otherwise has the preconditions and errors of the family's own call.  An allocation failure (KMPGPU_ENOMEM /
 * KMPGPU_EHIP) leaves the context usable and without flows.
 * Every other call is bit-identical, with the same launches and buffers, before and after any of these calls.
 * kmpgpu_flows_build: five kernels and two of the scan kernels kmpgpu_load_selected uses (insert, firsts, scan x 2, number, assign; the
 * total read once on the host in between), in the scratch the context keeps for those; *t (may be NULL): kernel_ms over all of them,
 * launches = 6.
 * Memory, all owned by the context, grown like the other buffers and freed by kmpgpu_destroy: the table and first[],
 * 4 bytes per slot each (slots: KMPGPU_OPT_FLOW_SLOTS); slot_of / flow_of, one array of 4 bytes per payload; the records, 48 bytes per
 * flow; the folded matrix, (rows x Sf + rows + Sf) x 8 bytes with Sf = 2 ceil(Wf / 2) (SCOPE_FLOW: rows = terms + rules); the select
 * buffer, (W + Wf) x 8 bytes. */
#define KMPGPU_FLOW_DIRECTED 1u
typedef struct kmpgpu_flow {          /* 48 bytes */
    uint64_t first_packet, last_packet;   /* payload indices */
    uint64_t n_packets;
    uint64_t payload_bytes;               /* sum of L_k */
    kmpgpu_pkt_meta first;                /* meta[first_packet] */
} kmpgpu_flow;
int  kmpgpu_flows_build(kmpgpu_ctx *ctx, uint32_t flags, uint64_t *n_flows /* or NULL */, kmpgpu_timing *t /* or NULL */);
int  kmpgpu_flows_read(kmpgpu_ctx *ctx, kmpgpu_flow *out, uint64_t first, uint64_t n);
int  kmpgpu_flow_ids_read(kmpgpu_ctx *ctx, uint32_t *out /* flow_of[first .. first + n) */, uint64_t first, uint64_t n);
#define KMPGPU_FLOW_SCOPE_PACKET 0u
#define KMPGPU_FLOW_SCOPE_FLOW   1u
int  kmpgpu_scan_flows(kmpgpu_ctx *ctx, int family /* KMPGPU_ALERT_* */, uint32_t scope, uint64_t *flow_counts_out /* [rows] or NULL */,
                       uint64_t *any_out /* [Wf] or NULL */, uint64_t *flow_hits_out /* [rows * Wf] or NULL */,
                       uint64_t *counts_out /* [n_pat] or NULL: as kmpgpu_scan */, kmpgpu_timing *t /* or NULL */);
int  kmpgpu_flows_select(kmpgpu_ctx *ctx, const void *flow_bits /* uint64_t[Wf] */, int on_device, uint64_t *pkt_bits_out /* host [W] or NULL */,
                         const void **d_pkt_bits /* or NULL */);

/* Flow seams: contents split across two payloads of a flow.  A per-payload matcher is walked past by cutting a content in two ("GET /adm"
 * ends one TCP segment, "in HTTP/1.1" starts the next): "/admin" hits in neither payload, and no flow-scope rule that names it fires.  The
 * overlap construction closes that gap without reassembly: for every payload that has a predecessor in its flow and direction, a SEAM -- a
 * small payload made of the predecessor's last `reach` bytes followed by this payload's first `reach` bytes -- goes into a packed arena
 * that a second context owns, and everything the library has scans the seams.  A pattern of up to reach + 1 bytes that straddles the
 * boundary lies inside the seam.
 * Definitions.  src holds built flows (kmpgpu_flows_build); e_src, e_dst, flow_of and kmpgpu_flow.first as defined there.
 *     dir(k)  = 0 where payload k's (e_src, e_dst) equal those of its flow's first payload (kmpgpu_flow.first), else 1.  Under
 *               KMPGPU_FLOW_DIRECTED it is always 0, and a flow whose two endpoints are equal has dir 0 throughout.
 *     pred(k) = the largest j < k with flow_of[j] == flow_of[k] and dir(j) == dir(k): a TCP stream is per direction, so an undirected flow
 *               has two chains.  A payload without a predecessor has no seam.
 * Seams are numbered in ascending order of `next`.  With prev = pred(next), tail_len = min(reach, L_prev), head_len = min(reach, L_next)
 * (the index's lengths, whatever KMPGPU_OPT_WHOLE_PAYLOAD says), seam j is the raw bytes
 *     payload_prev[L_prev - tail_len : L_prev] ++ payload_next[0 : head_len]
 * There is one seam per payload with a predecessor, also when it comes to 0 bytes (an empty payload owning one zero slot), so
 * n_seams == n_pkts - (number of distinct (flow, dir)).  The order is capture order, not sequence numbers, and no atomic decides it: the
 * arena and every record are byte-identical from run to run.  reach is 1 .. KMPGPU_MAX_PATTERN_LEN - 1 = 98.
 *
 * kmpgpu_load_seams.  dst ends up in the state kmpgpu_load_selected leaves it in: an owned packed arena of the n_seams seams, slots of
 * max(16, round_up(len, 16)) bytes back to back from offset 0, 0x00 behind every seam's end, padding known clean, packet-start bitmap and
 * plans rebuilt, the nocase fold stale.  dst gets metadata, meta[j] = src.meta[next_j] (header predicates of dst's rules see the segment
 * the seam leads into), and keeps the records kmpgpu_seam[n_seams] and seam_flow[j] = src.flow_of[next_j] in device buffers it owns;
 * kmpgpu_seams_read copies records [first, first + n) to out, ranges and errors as kmpgpu_flows_read.  Whatever replaces or releases dst's
 * arena (kmpgpu_load_arena, kmpgpu_attach_arena, kmpgpu_load_frames, kmpgpu_load_selected and kmpgpu_load_seams as dst) drops the seam
 * state; the buffers stay for the next build.  *n_seams (may be NULL) = the number of seams.  n_pkts == 0, or no seam at all (every flow
 * direction a single payload): dst is left without an arena, the call returns KMPGPU_OK with *n_seams = 0, and an empty seam list exists.
 * Untouched: src is not written, and every output of it is bit-identical before and after.  The source is whatever src scans now (loaded,
 * attached, extracted, repacked or kept in place).  Of its arena no byte outside the slots of prev and next is read: the gather loads
 * aligned 16-byte units that hold a byte of a tail or a head, so a borrowed arena owes nothing behind its last slot.
 * A SEAM IS A PAYLOAD OF ITS OWN.  dst scans it under dst's own patterns, flags, windows (offsets count from the seam's first byte) and E
 * rule.  Under the default strlen rule a 0x00 in the seam ends the seam's text; a 0x00 in prev more than `reach` bytes in front of prev's
 * end is not seen, so the seam rows may hold a match that lies in prev's bytes behind prev's first 0x00 -- bytes src's own scan never
 * reaches.  Under KMPGPU_OPT_WHOLE_PAYLOAD on both contexts the seam rows hold nothing that the concatenated stream does not hold.
 * Ordering: synchronous.  Waits for dst's stream and for src's, as kmpgpu_load_selected does, and works on dst's stream; the scratch is
 * the one dst keeps for kmpgpu_load_frames plus a sort buffer of its own (24 bytes per source payload and rocPRIM's temporary storage).
 * Errors: dst == src, a NULL context, reach outside 1 .. 98, contexts on different devices: KMPGPU_EINVAL; src without built flows:
 * KMPGPU_ESTATE ("no flows"); either context between kmpgpu_load_frames_begin and _finish: KMPGPU_ESTATE; after each of these dst keeps its
 * arena.  After an allocation failure (KMPGPU_ENOMEM / KMPGPU_EHIP) dst is without an arena and both contexts stay usable.
 * kmpgpu_last_timing(dst): kernel_ms from the keys kernel to the gather's end (the host's read of the totals lies inside), launches = 7
 * (keys, the sort counted as one, pred, two scan kernels, index, gather; 5 where there is no seam).  Under kmpgpu_profile_begin on dst the
 * entries are keys, sort, pred + the two scan kernels, index, gather.
 *
 * kmpgpu_scan_flows_seams(src, seams, ...) is kmpgpu_scan_flows(src, KMPGPU_ALERT_RULES, KMPGPU_FLOW_SCOPE_FLOW, ...) with one step added:
 * before the rules kernel, the pattern rows of a marking pass over `seams` (the pass of kmpgpu_scan_packets(seams), on seams' stream, which
 * the call waits for as kmpgpu_counts_add does) are folded into the same folded matrix through seam_flow, by the fold kernel a second time:
 *     term[i][f] = OR over the payloads k of flow f of hit_src[i][k]  |  OR over the seams j of flow f of hit_seams[i][j]      (i < n_pat)
 * Relation, chain, header and byte-test terms stay src's own, and counts_out stays what kmpgpu_scan(src) returns: cross-boundary matches are not
 * counted.  One boundary per seam: a content that spans three payloads is not found.  Outputs and layout as kmpgpu_scan_flows.
 * Preconditions: `seams` holds a seam list built from src's CURRENT flows (every kmpgpu_flows_build and everything that drops the flows
 * starts a new generation; a list of another generation or another context: KMPGPU_ESTATE), both contexts sit on one device (otherwise
 * KMPGPU_EINVAL) and hold the same pattern bytes and flags (otherwise KMPGPU_ESTATE); everything else as kmpgpu_scan_flows on src and as
 * kmpgpu_scan_packets on seams.  *t: as kmpgpu_scan_flows, launches = what kmpgpu_scan_flows reports + what kmpgpu_scan_packets(seams)
 * reports + 1 (the second fold).  With an empty seam list the call returns exactly what kmpgpu_scan_flows(SCOPE_FLOW) returns, launches
 * included.
 * Every existing call keeps its outputs, launches and buffers, with or without these calls having run.
 * Cost (the figures of tools/seams.py go to profiles/seams.txt): 24 bytes per source payload sorted, one read of the two
 * slots' ends per seam, 2 x reach bytes written per seam; the scan of the seams is a scan of n_seams small payloads. */
typedef struct kmpgpu_seam {        /* 24 bytes */
    uint64_t prev, next;            /* payload indices in src: the seam joins the end of prev to the start of next */
    uint32_t tail_len, head_len;    /* min(reach, L_prev), min(reach, L_next); the seam payload is tail_len + head_len bytes */
} kmpgpu_seam;
int  kmpgpu_load_seams(kmpgpu_ctx *dst, kmpgpu_ctx *src, uint32_t reach, uint64_t *n_seams /* or NULL */);
int  kmpgpu_seams_read(kmpgpu_ctx *dst, kmpgpu_seam *out, uint64_t first, uint64_t n);
int  kmpgpu_scan_flows_seams(kmpgpu_ctx *src, kmpgpu_ctx *seams, uint64_t *flow_counts_out /* [n_rules] or NULL */,
                             uint64_t *any_out /* [Wf] or NULL */, uint64_t *flow_hits_out /* [n_rules * Wf] or NULL */,
                             uint64_t *counts_out /* [n_pat] or NULL: as kmpgpu_scan(src) */, kmpgpu_timing *t /* or NULL */);

/* Flow streams: the payloads of every direction of every flow reassembled.  A signature is written against the byte stream of one direction
 * of a connection, and the matcher sees segments: a content cut into three segments, or a stream of one-byte segments, walks past every
 * content rule, and a seam (above) holds one boundary and pattern rows only.  kmpgpu_load_streams concatenates the payloads of every
 * (flow, direction) of src, in capture order, into ONE payload each of a packed arena that a second context owns.  A stream is then an
 * ordinary payload of an ordinary context: patterns, counts, offsets, windows, relations, chains, byte tests, regex rows, rules, alerts,
 * kmpgpu_load_decoded and kmpgpu_load_selected run over it as over any other.
 * Definitions.  src holds built flows (kmpgpu_flows_build); flow_of and dir(k) exactly as the seams section defines them.  A STREAM is one
 * distinct (flow_of, dir) of src; streams are numbered in ascending order of flow << 1 | dir, so n_streams == n_pkts - n_seams.  Its members
 * are the payloads of that flow and direction in capture order (a stable sort; not sequence numbers), and no atomic decides anything: the
 * arena and every record are byte-identical from run to run.  With L_k the index's lengths, whatever KMPGPU_OPT_WHOLE_PAYLOAD says, stream s
 * is the raw bytes
 *     payload_k0[0 : L_k0] ++ payload_k1[0 : L_k1] ++ ...          over its members k0 < k1 < ...,
 * cut to its first `depth` bytes, depth in 1 .. KMPGPU_STREAM_DEPTH_MAX = 2^30 (which keeps every offset inside a stream below 2^31, as the
 * relation and chain arithmetic and pkt_len need).  A member that starts at or behind the cut contributes nothing but still has its map
 * entry.  A stream of 0 bytes exists and owns one zero slot.
 *
 * kmpgpu_load_streams.  dst ends up in the state kmpgpu_load_selected leaves it in: an owned packed arena of the n_streams streams, slots of
 * max(16, round_up(len, 16)) bytes back to back from offset 0, 0x00 behind every stream's end, padding known clean, packet-start bitmap and
 * plans rebuilt, the nocase fold stale.  dst gets metadata, meta[s] = src.meta[first_packet_s], and keeps the records kmpgpu_stream[n_streams]
 * and the map kmpgpu_stream_pos[n_pkts of src] in device buffers it owns; kmpgpu_streams_read / kmpgpu_stream_map_read copy elements
 * [first, first + n) to out, ranges and errors as kmpgpu_flows_read ("no streams": KMPGPU_ESTATE).  Whatever replaces or releases dst's
 * arena drops the stream state; the buffers stay for the next build.  *n_streams (may be NULL) = the number of streams.  n_pkts == 0: dst
 * is left without an arena, the call returns KMPGPU_OK with *n_streams = 0, and empty records exist.
 * Untouched: src is not written, and every output of it is bit-identical before and after.  The source is whatever src scans now (loaded,
 * attached, extracted, repacked or kept in place).  Of its arena no byte outside a member's slot is read: the gather loads aligned 16-byte
 * units that hold a byte of a member, so a borrowed arena owes nothing behind its last slot.
 * A STREAM IS A PAYLOAD OF ITS OWN.  dst scans it under dst's own patterns, flags, windows and E rule.  Under the default strlen rule its
 * text ends at the stream's first 0x00, wherever in the connection that lies.  Windows count from the stream's first byte: on a stream they
 * mean "offset in the connection's direction".  With KMPGPU_OPT_WHOLE_PAYLOAD on both contexts the stream holds every match src holds
 * inside the cut, plus the ones that cross member boundaries.
 * THE FLOW IDENTITY.  After kmpgpu_load_streams(dst, src, ...), kmpgpu_flows_build(dst, flags) with the flag src's flows were built with
 * gives flow_of_dst[s] == stream[s].flow for every s and the same n_flows: flows are numbered by their first payload, dst's order is
 * (flow, dir), and every flow has a dir-0 stream whose metadata is the flow's `first`.  So kmpgpu_scan_flows(dst, KMPGPU_ALERT_RULES,
 * KMPGPU_FLOW_SCOPE_FLOW, ...) is the reassembled flow-scope verdict in src's flow numbering; there is no further fold call.
 * Ordering: synchronous.  Waits for dst's stream and for src's, as kmpgpu_load_seams does, and works on dst's stream; the scratch is the
 * one dst keeps for kmpgpu_load_frames (grown to 40 bytes per source payload for the scans, 24 for the gather's piece records) and the
 * sort buffer of kmpgpu_load_seams.  The host reads device totals twice: {member bytes, n_streams}, which size the records, then the packed
 * arena's bytes, which follow from the cut lengths.
 * Errors: dst == src, a NULL context, depth outside 1 .. 2^30, contexts on different devices: KMPGPU_EINVAL; src without built flows:
 * KMPGPU_ESTATE ("no flows"); either context between kmpgpu_load_frames_begin and _finish: KMPGPU_ESTATE; after each of these dst keeps its
 * arena.  After an allocation failure (KMPGPU_ENOMEM / KMPGPU_EHIP) dst is without an arena and both contexts stay usable.
 * kmpgpu_last_timing(dst): kernel_ms from the keys kernel to the gather's end (the host's two reads lie inside), launches = 10 (keys, the
 * sort counted as one, stream scan, stream totals, heads, records, the two slot scan kernels, index, gather).  Under kmpgpu_profile_begin on
 * dst the entries are keys, sort, stream scan + totals, heads + records + the two slot scan kernels, index, gather.
 * Every existing call keeps its outputs, launches and buffers, with or without these calls having run.
 * Not done here: capture order, not sequence numbers; a retransmitted segment appears twice (kmpgpu_load_streams_ordered below does both).
 * Not done: no TCP state, no timeouts; one cut per stream; streams are per context, not across shards or GPUs. */
#define KMPGPU_STREAM_DEPTH_MAX (1u << 30)
typedef struct kmpgpu_stream {        /* 48 bytes */
    uint64_t first_packet, last_packet;   /* src payload indices of the stream's first and last member */
    uint64_t n_packets;                   /* members */
    uint64_t bytes;                       /* sum of the members' L_k, before the depth cut */
    uint32_t flow, dir;                   /* src.flow_of[first_packet], dir() as kmpgpu_load_seams defines it */
    uint32_t len, reserved;               /* min(bytes, depth): the stream payload's length in dst; 0 */
} kmpgpu_stream;
typedef struct kmpgpu_stream_pos {    /* 16 bytes, one per SOURCE payload */
    uint32_t stream, reserved;            /* the stream payload k belongs to; 0 */
    uint64_t pos;                         /* sum of L_j over the members j < k of that stream: where k's first byte lies, before the cut */
} kmpgpu_stream_pos;
int  kmpgpu_load_streams(kmpgpu_ctx *dst, kmpgpu_ctx *src, uint32_t depth, uint64_t *n_streams /* or NULL */);
int  kmpgpu_streams_read(kmpgpu_ctx *dst, kmpgpu_stream *out, uint64_t first, uint64_t n);
int  kmpgpu_stream_map_read(kmpgpu_ctx *dst, kmpgpu_stream_pos *out, uint64_t first, uint64_t n);

/* Flow streams by TCP sequence number.  kmpgpu_load_streams keeps capture order: one reordered segment leaves "GET /admin" not contiguous, a
 * retransmitted segment makes a content count twice and moves every later offset, window, chain distance and byte test.
 * kmpgpu_load_streams_ordered(dst, src, depth, seq, on_device, n_streams) is its sibling with one 32-bit TCP sequence number per source
 * payload: seq is uint32_t[n_pkts of src], in host memory (on_device == 0) or in device memory on the contexts' device (on_device == 1,
 * complete before the call), borrowed for the call.  It builds the streams of TCP flows in sequence order, with bytes already delivered
 * dropped and holes closed.  Streams, their numbering (flow << 1 | dir), dir(k), the slot layout, depth, the metadata (meta[s] =
 * src.meta[first_packet_s], first_packet the first member IN CAPTURE ORDER), the flow identity, the state dst is left in, what is untouched
 * and the ordering are exactly those of kmpgpu_load_streams.
 * Definitions.  A stream is a TCP stream iff src.meta[first_packet_s].proto == 6.  Every other stream is built exactly as
 * kmpgpu_load_streams builds it: capture order, skip = 0, take = L_k.  For a TCP stream with members k0 < k1 < ... in capture order:
 *     rel(k)  = (int32_t)(uint32_t)(seq[k] - seq[k0])      two's complement: serial-number arithmetic around the first captured member
 *     off(k)  = rel(k) - min over the members j of rel(j)  in [0, 2^32): the member's offset in the stream's sequence space
 *     order   = ascending (off(k), k)                      equal sequence numbers stay in capture order
 *     byte x  = payload_k[x - off(k)] of the FIRST k in that order with off(k) <= x < off(k) + L_k
 *     stream  = the bytes of all covered x in ascending x, holes closed (nothing is written for an uncovered x), cut to its first `depth`
 *               bytes
 * Per member, with M(k) the maximum of off(j) + L_j over the members before k in the order (0 for the first): skip(k) = min(L_k,
 * max(0, M(k) - off(k))), take(k) = L_k - skip(k), pos(k) = the sum of take over the members before it, before the cut.  The kept bytes
 * of a member are always a suffix of it, because every earlier member starts at or before it.  A member other than the first with
 * off(k) > M(k) opens a gap of off(k) - M(k) bytes.  First in sequence order wins: that is the only overlap policy.
 * No TCP flags are read: a SYN's phantom byte is a 1-byte gap, a reused 5-tuple interleaves its connections by sequence number.  A stream
 * whose members span 2^31 or more of sequence space is computed by the arithmetic above, and nothing more is promised for it.
 * Records.  kmpgpu_stream is unchanged: bytes is the sum of take, n_packets all members, first_packet / last_packet in capture order.
 * kmpgpu_stream_pos is unchanged: pos is the position of the member's first kept byte.  New: kmpgpu_stream_seg[n_pkts of src], one per
 * source payload, and kmpgpu_stream_order[n_streams]; kmpgpu_stream_segs_read / kmpgpu_stream_orders_read copy elements [first, first + n)
 * to out, ranges and errors as kmpgpu_streams_read, and return KMPGPU_ESTATE after a plain kmpgpu_load_streams ("no sequence order").
 * No atomic decides a value: two builds are byte-identical.
 * Scratch: that of kmpgpu_load_streams, a workspace of its own for the second sort and the scans (40 bytes per source payload plus
 * rocPRIM's temporary storage), and, with on_device == 0, a device copy of seq; all kept by dst for the next build.
 * Errors: those of kmpgpu_load_streams, plus seq == NULL with n_pkts > 0, on_device outside {0, 1}, n_pkts > 2^30 (which keeps the
 * composite sort keys inside 64 bits): KMPGPU_EINVAL; src without metadata: KMPGPU_ESTATE.  After each of these dst keeps its arena.
 * kmpgpu_last_timing(dst): kernel_ms from the keys kernel to the gather's end (the upload of a host seq lies before it, the host's two
 * reads inside), launches = 16 (keys, the sort, stream scan, stream totals, heads, second keys, the second sort, maximum scan, maximum
 * totals, take scan, take totals, records, the two slot scan kernels, index, gather).  Under kmpgpu_profile_begin on dst the entries are
 * keys, sort, stream scan + totals, heads + second keys + second sort, the four scan kernels, records + the two slot scan kernels, index,
 * gather.
 * Not done: no TCP state or flags, no timeouts; one cut per stream; per context; kmpgpu_load_frames keeps no sequence
 * numbers (kmphost's kmp_arena_from_pcap_seq does); no overlap policy but first-in-sequence-order. */
typedef struct kmpgpu_stream_seg {    /* 16 bytes, one per SOURCE payload */
    uint32_t skip, take;                  /* bytes of k already delivered by earlier members; L_k - skip, before the cut */
    uint32_t seq_off, reserved;           /* off(k); 0 for a member of a stream that is not TCP.  0 */
} kmpgpu_stream_seg;
typedef struct kmpgpu_stream_order {  /* 32 bytes, one per stream */
    uint32_t seq_base, n_gaps;            /* the sequence number of offset 0 (the lowest of the stream); members that open a gap */
    uint64_t gap_bytes, dup_bytes;        /* sum of the gaps; sum of skip */
    uint32_t tcp, reserved;               /* 1: built in sequence order; 0: capture order, and every other field 0.  0 */
} kmpgpu_stream_order;
int  kmpgpu_load_streams_ordered(kmpgpu_ctx *dst, kmpgpu_ctx *src, uint32_t depth, const uint32_t *seq, int on_device,
                                 uint64_t *n_streams /* or NULL */);
int  kmpgpu_stream_segs_read(kmpgpu_ctx *dst, kmpgpu_stream_seg *out, uint64_t first, uint64_t n);
int  kmpgpu_stream_orders_read(kmpgpu_ctx *dst, kmpgpu_stream_order *out, uint64_t first, uint64_t n);

/* ---- flow bits: rule state carried along a flow's payloads (the `flowbits` of signature languages) --------------------------------------
 * kmpgpu_set_flowbits gives rules of kmpgpu_set_rules tests and actions on n_bits state bits per flow; kmpgpu_scan_flowbits evaluates
 * them over the built flows (kmpgpu_flows_build, directed or not, exactly as built) in capture order.
 *
 * Definition.  An op is (rule, bit, op): KMPGPU_FB_ISSET / KMPGPU_FB_ISNOTSET are tests, KMPGPU_FB_SET / _UNSET / _TOGGLE actions,
 * KMPGPU_FB_NOALERT marks the rule (bit ignored).  base[r][k] is the bit kmpgpu_scan_rules defines.  For every flow f with the payloads
 * k_1 < k_2 < ... and a 32-bit state S that starts at 0, payload after payload:
 *   1. B = S, the state BEFORE k_j;
 *   2. fired[r][k_j] = base[r][k_j] AND every test of rule r holds on B -- all rules of a payload see the same B;
 *   3. S = B changed by the actions of the fired rules, rules in ascending index, a rule's actions in the order they were given;
 *   4. alert[r][k] = fired[r][k] AND rule r has no KMPGPU_FB_NOALERT.
 * So a bit a rule sets is seen by testers from the NEXT payload of the flow on, never in the same payload: the one deliberate difference
 * from engines that order setters before checkers inside a packet, and what makes the state a scan.  `isnotset X; set X` fires exactly once
 * per flow; two flows never share state; under KMPGPU_FLOW_DIRECTED the two directions of a conversation are two flows and two states.
 *
 * How it is parallel.  For one bit a payload's effect is a function {0,1} -> {0,1}, two bits (F(0), F(1)); a rule may test the very bit it
 * changes, which is F depending on its argument.  Functions compose associatively, so the states before every payload are a scan of
 * compositions in flow order, restarted at every flow's first payload.  Across different bits there is an edge Y -> X where some rule tests
 * Y and acts on X, Y != X; this graph must be acyclic (KMPGPU_EINVAL otherwise, the bits of a cycle named in the message), level(X) is the
 * longest path into X, and the bits are decided level by level, the lower levels' states known.
 *
 * kmpgpu_set_flowbits(ctx, ops, n_ops, n_bits): n_ops == 0 clears (ops and n_bits are not looked at).  KMPGPU_ESTATE without rules.
 * KMPGPU_EINVAL, with the ops set before still in force: n_bits outside 1..KMPGPU_FLOWBITS_MAX, ops NULL, a rule >= n_rules, a bit >= n_bits
 * (not for NOALERT), an unknown op, a nonzero reserved field, the same (rule, bit) tested both ways, a cycle.  Whatever drops the rules
 * (kmpgpu_set_patterns, every setter that drops them) and every successful kmpgpu_set_rules drops the ops, whose rule indices meant those
 * rules; kmpgpu_flows_build keeps them.
 *
 * kmpgpu_scan_flowbits: every output may be NULL.  rule_pkt_counts_out[r] = set bits of alert row r, any_out[W] the OR of the alert rows,
 * rule_hits_out[n_rules * W] the alert rows (a NOALERT rule's row is 0 and adds nothing), state_out[n_bits * W]: bit k of row X = bit X of
 * the state before payload k, flow_state_out[n_flows]: S after the flow's last payload, counts_out as kmpgpu_scan.  W = ceil(n_pkts / 64),
 * bits at n_pkts and above are 0.  KMPGPU_ESTATE: no patterns, no arena, no rules, "no flow bits", "no flows" (none built since the arena
 * or its metadata were set), between kmpgpu_load_frames_begin and _finish; the header predicates' "no packet metadata".  With n_pkts == 0
 * every count is 0 and nothing is launched.  Results do not depend on the run: no atomic decides a value, and no block waits on another.
 *
 * Launches.  The pass of kmpgpu_scan_rules, unchanged.  Once per build of the flows (cached by flow generation): a stable rocPRIM radix
 * sort of (flow_of[k], k) over the flow ids' significant bits, and one kernel for the inverse order and the head flags.  Per level four
 * steps: build (a lane per payload: 8 bytes (f0 mask, f1 mask), stored at the payload's sorted position; a flow's first payload stores the
 * constant function (F(0), F(0)), which is the restart), the scan -- tiles of KMP_SCAN_TILE reduced to one aggregate each, the aggregates
 * scanned by the same kernels, recursively, then every tile scanned from its carry-in (one kernel where n_pkts <= KMP_SCAN_TILE) --, which
 * scatters the state before every payload and writes flow_state at every flow's last, and the rows kernel (one ballot per bit of the level).
 * Last the final pass: alert[r] = base[r] AND the tests, word-wise, with counts and any[].  t->launches counts all of them.
 * Memory, kept by the context: 13 bytes per payload for the order, rocPRIM's temporary storage, 12 bytes per payload and 8 per tile for
 * the scan, 4 per flow, the before rows [n_bits][stride] and the alert rows [n_rules][stride] (stride = 2 ceil(W / 2) words).  An allocation
 * failure is KMPGPU_ENOMEM and leaves the context usable.
 * Not done: no KMPGPU_ALERT_* family, so kmpgpu_scan_alerts / kmpgpu_scan_flows know nothing of flow bits; no seams or streams. */
#define KMPGPU_FLOWBITS_MAX 32
#define KMPGPU_FB_ISSET    0
#define KMPGPU_FB_ISNOTSET 1
#define KMPGPU_FB_SET      2
#define KMPGPU_FB_UNSET    3
#define KMPGPU_FB_TOGGLE   4
#define KMPGPU_FB_NOALERT  5
typedef struct kmpgpu_flowbit_op { uint32_t rule, bit, op, reserved; } kmpgpu_flowbit_op;
int  kmpgpu_set_flowbits(kmpgpu_ctx *ctx, const kmpgpu_flowbit_op *ops, uint32_t n_ops, uint32_t n_bits);
int  kmpgpu_scan_flowbits(kmpgpu_ctx *ctx, uint64_t *rule_pkt_counts_out /* [n_rules] or NULL */, uint64_t *any_out /* [W] or NULL */,
                          uint64_t *rule_hits_out /* [n_rules * W] or NULL */, uint64_t *state_out /* [n_bits * W] or NULL */,
                          uint32_t *flow_state_out /* [n_flows] or NULL */, uint64_t *counts_out /* [n_pat] or NULL */,
                          kmpgpu_timing *t /* or NULL */);

/* ---- rate thresholds: a rule fires on the Nth hit per tracker in a time window (`detection_filter`, `threshold` of signature languages) --
 * kmpgpu_set_thresholds gives rules of kmpgpu_set_rules conditions on how often they have hit per source, destination, flow or altogether;
 * kmpgpu_scan_thresholds evaluates them with one timestamp per payload from the caller.
 *
 * Definition.  ts[k] is an unsigned 64-bit time in a unit the library does not know; a threshold's `window` is in the same unit.  Time
 * never runs backwards for the engine: T[k] = max(ts[0 .. k]) in capture order.  A threshold q is (rule r, track, type, count, window);
 * base[r][k] is the bit kmpgpu_scan_rules defines.  tracker(q, k) is 0 under KMPGPU_THR_BY_RULE (one tracker), meta[k].src_ip under
 * KMPGPU_THR_BY_SRC, meta[k].dst_ip under KMPGPU_THR_BY_DST, flow_of[k] of the built flows under KMPGPU_THR_BY_FLOW (it follows
 * KMPGPU_FLOW_DIRECTED exactly as built).
 *   n[q][k]     = #{ j <= k : tracker(q, j) == tracker(q, k), base[r][j] == 1, T[k] - T[j] < window }
 *   pass[q][k]  = n >= count (KMPGPU_THR_AT_LEAST) | n <= count (KMPGPU_THR_AT_MOST) | n == count (KMPGPU_THR_EXACTLY)
 *   alert[r][k] = base[r][k] AND pass[q][k] for every threshold q on rule r          (a rule without thresholds: alert = base)
 * window == KMPGPU_THR_NO_WINDOW means every j <= k of the tracker.  j <= k is capture order: of two payloads with equal T only the
 * earlier one counts for the other, and a payload counts itself when it hits.
 * THESE ARE SLIDING WINDOWS OVER THE RULE'S BASE HITS: not the tumbling windows of Snort's implementation, and they do not count issued
 * alerts.  This is the one deliberate difference, the counterpart of flow bits' "seen from the next payload on", and what makes the count
 * a prefix sum plus a search.  KMPGPU_THR_AT_MOST c therefore reads: the first c hits of a burst, armed again once the window holds fewer
 * than c.
 *
 * kmpgpu_set_thresholds(ctx, thr, n_thr): n_thr == 0 clears (thr is not looked at).  KMPGPU_ESTATE without rules.  KMPGPU_EINVAL, with the
 * thresholds set before still in force: thr NULL, a rule >= n_rules, an unknown track or type, count == 0, window == 0.  Whatever drops the
 * rules and every successful kmpgpu_set_rules drops the thresholds; kmpgpu_flows_build keeps them.
 *
 * kmpgpu_scan_thresholds: every output may be NULL.  rule_pkt_counts_out[r] = set bits of alert row r, any_out[W] the OR of the alert rows,
 * rule_hits_out[n_rules * W] the alert rows, window_counts_out[n_thr * n_pkts]: n[q][k] for EVERY k, also where base[r][k] is 0 (the
 * payload itself then adds nothing), counts_out as kmpgpu_scan.  W = ceil(n_pkts / 64), bits at n_pkts and above are 0.  ts_on_device is 0
 * or 1; 1: device memory on the context's device, 8-byte aligned.  KMPGPU_ESTATE: no patterns, no arena (no load call has reached the
 * context yet; an arena of zero payloads is one), no rules, "no thresholds", "no
 * packet metadata" (only when a BY_SRC or BY_DST threshold is set, or the rules hold header predicates), "no flows" (only when a BY_FLOW
 * threshold is set), between kmpgpu_load_frames_begin and _finish.  KMPGPU_EINVAL: ts NULL with n_pkts > 0, another ts_on_device, device
 * timestamps that are not 8-byte aligned.  With
 * n_pkts == 0 every count is 0 and nothing is launched.  Results do not depend on the run: no atomic decides a value, and no block waits on
 * another.
 *
 * Launches.  The pass of kmpgpu_scan_rules, unchanged.  The timestamps are copied into the context's buffer and max-scanned in place
 * (64-bit; tiles of KMP_SCAN_TILE reduced to one aggregate each, the aggregates scanned by the same kernels, recursively, then every tile
 * from its carry-in); skipped when every window is KMPGPU_THR_NO_WINDOW.  Per track in use an order: BY_FLOW the order of
 * kmpgpu_scan_flowbits and its cache per build of the flows; BY_SRC / BY_DST one kernel for the keys and a stable rocPRIM radix sort of
 * (address, k) over 32 bits with the inverse order and head flags, cached until the arena or its metadata change; BY_RULE the identity, no
 * sort and no buffer.  Per sorted track one kernel that puts T into the track's order.  Per threshold: gather the rule's bits into sorted
 * order, a 32-bit prefix sum (the same three-kernel scan), and the pass kernel -- a lane per payload, a binary search over (key, T) for the
 * window's first position, the comparison, one ballot per 64 payloads.  Last the final pass: alert[r] = base[r] AND its pass rows.
 * t->launches counts all of them.
 * Memory, kept by the context: 13 bytes per payload and rocPRIM's temporary storage per sorted track, 8 bytes per payload for T and 8 per
 * sorted track, 4 for the prefix sum, 8 per tile, the pass rows [n_thr][stride] and the alert rows [n_rules][stride] (stride =
 * 2 ceil(W / 2) words), 4 n_thr n_pkts bytes when window_counts_out is asked for.  An allocation failure is KMPGPU_ENOMEM and leaves the
 * context usable.
 * Not done: thresholds over flow-bit alerts; tracking by address pair; tumbling windows and counts of issued alerts; timestamps through
 * kmpgpu_load_frames, kmpgpu_load_selected or streams (the caller keeps them); no KMPGPU_ALERT_* family, so kmpgpu_scan_alerts /
 * kmpgpu_scan_flows know nothing of thresholds. */
#define KMPGPU_THR_BY_RULE  0
#define KMPGPU_THR_BY_SRC   1
#define KMPGPU_THR_BY_DST   2
#define KMPGPU_THR_BY_FLOW  3
#define KMPGPU_THR_AT_LEAST 0
#define KMPGPU_THR_AT_MOST  1
#define KMPGPU_THR_EXACTLY  2
#define KMPGPU_THR_NO_WINDOW (~0ull)
typedef struct kmpgpu_threshold { uint32_t rule, track, type, count; uint64_t window; } kmpgpu_threshold;   /* 24 bytes */
int  kmpgpu_set_thresholds(kmpgpu_ctx *ctx, const kmpgpu_threshold *thr, uint32_t n_thr);
int  kmpgpu_scan_thresholds(kmpgpu_ctx *ctx, const uint64_t *ts, int ts_on_device, uint64_t *rule_pkt_counts_out /* [n_rules] or NULL */,
                            uint64_t *any_out /* [W] or NULL */, uint64_t *rule_hits_out /* [n_rules * W] or NULL */,
                            uint32_t *window_counts_out /* [n_thr * n_pkts] or NULL */, uint64_t *counts_out /* [n_pat] or NULL */,
                            kmpgpu_timing *t /* or NULL */);

/* Linked rows: a row that ANOTHER context computed as one more row of this context's hit matrix, and so one more rule term (DESIGN.md
 * §3.33).  The derived arenas -- kmpgpu_load_decoded, _base64, _fields, _dns, _streams, _selected -- each hold another view of the same
 * payloads in a context of their own; a link carries a verdict on that view back into the context whose rules want it, translated on the
 * device into this context's payload numbering.  Everything that starts from the rules' rows (kmpgpu_scan_rules, kmpgpu_scan_alerts,
 * kmpgpu_scan_flows, kmpgpu_scan_flowbits, kmpgpu_scan_thresholds, kmpgpu_scan_flows_seams) then works on rules over several buffers.
 *
 * kmpgpu_set_links reserves n_links rows behind the expressions' rows: link q is row and rule term
 * n_pat + n_rel + n_chains + n_hdr + n_bt + n_rx + q, with or without KMPGPU_RULE_NOT.  Like every family setter it needs patterns set
 * (KMPGPU_ESTATE) and drops the rules, and with them the flow bits and thresholds; n_pat + ... + n_links >= 2^31 is KMPGPU_EINVAL, here
 * and in every family setter called while links are set.
 * n_links = 0 clears the family; kmpgpu_set_patterns drops the links as it drops the other families.  Every link starts unfilled.
 *
 * kmpgpu_link_rows fills links first_link .. first_link + n_rows - 1 of dst from rows first_row .. first_row + n_rows - 1 of src's family
 * (KMPGPU_ALERT_*: patterns, rules, relations, chains).  It runs src's pass for that family itself -- the marking pass and the family's
 * kernels, what kmpgpu_scan_<family> with every output NULL runs -- and leaves src as that call leaves it.  Then one kernel translates the
 * rows into the link buffer dst owns, [n_links][stride]: bit k of a link row is 1 exactly where k < n_dst, map(k) exists and bit map(k) of
 * src's row is 1; the bits at n_dst and above and the padding word of an odd W are 0.  The map kinds:
 *   KMPGPU_LINK_SAME    payload k of src is payload k of dst; n_src != n_dst: KMPGPU_EINVAL; map is not read.
 *   KMPGPU_LINK_BITMAP  map = uint64_t[ceil(n_dst / 64)]: the j-th set bit below n_dst is src's payload j -- the d_changed / d_present
 *                       pointers and the select bitmap as they are.  Bits at n_dst and above are ignored; a popcount below n_dst that
 *                       is not n_src: KMPGPU_EINVAL.  On the device the map is 8-byte aligned.
 *   KMPGPU_LINK_INDEX   map = uint32_t[n_dst]: src's payload for dst's payload k; a value >= n_src (KMPGPU_LINK_NONE): none.  Many
 *                       payloads may name one: a payload takes the verdict of its stream or of its seam.
 * map_on_device: 0 a host array, copied; 1 a device array of dst's device, complete before the call.  src without payloads fills zeros.
 * src's family may be KMPGPU_ALERT_RULES, and its rules may name src's own links: links chain.
 * Synchronous: it waits for both contexts' streams, as kmpgpu_load_selected does.  t: kernel_ms is the translation alone, by events of
 * its own on dst's stream -- the rank kernels of a bitmap plus the gather --, launches their number; src's pass is in neither.
 * KMPGPU_EINVAL: a NULL context; dst == src (rules of rules do not exist); contexts on two devices; a family that is none of
 * KMPGPU_ALERT_*, a map kind that is none of KMPGPU_LINK_*; a row or a link range out of bounds; KMPGPU_LINK_SAME with unequal payload
 * counts; a NULL map where one is read; map_on_device not 0 or 1; a misaligned device map.  KMPGPU_ESTATE: either context between
 * kmpgpu_load_frames_begin and _finish; dst without an arena; what src's own call for the family refuses.  After any error dst's links are
 * what they were: the filled ones hold their rows, the others read as zeros.
 * A link stays filled until dst's arena changes (every load, attach and derived-arena loader) or kmpgpu_set_links is called again; src may
 * change freely afterwards, the caller links again when it wants the new verdict.  A pass over rules that name an unfilled link --
 * kmpgpu_scan_rules, kmpgpu_scan_alerts and kmpgpu_scan_flows of the rules, kmpgpu_scan_flowbits, kmpgpu_scan_thresholds,
 * kmpgpu_scan_flows_seams -- is KMPGPU_ESTATE and names the link.  Behind the marking pass the link buffer is copied into the matrix (one
 * device-to-device copy); no existing kernel changes.
 *
 * kmpgpu_scan_links: the family's own scan call, as kmpgpu_scan_regexes: the marking pass, the copy and the reduce of kmpgpu_scan_packets
 * over the link rows.  An unfilled link reads as zeros.  No links set: KMPGPU_ESTATE.
 * Not done: links to a context's own rows; rows in flow space (kmpgpu_scan_flows results) as a source; links across devices; automatic
 * refill when src changes; match offsets. */
#define KMPGPU_LINK_SAME    0
#define KMPGPU_LINK_BITMAP  1
#define KMPGPU_LINK_INDEX   2
#define KMPGPU_LINK_NONE    0xFFFFFFFFu
int  kmpgpu_set_links(kmpgpu_ctx *ctx, uint32_t n_links);
int  kmpgpu_link_rows(kmpgpu_ctx *dst, uint32_t first_link, kmpgpu_ctx *src, int family /* KMPGPU_ALERT_* */, uint32_t first_row,
                      uint32_t n_rows, int map_kind /* KMPGPU_LINK_* */, const void *map, int map_on_device, kmpgpu_timing *t /* or NULL */);
int  kmpgpu_scan_links(kmpgpu_ctx *ctx, uint64_t *link_pkt_counts_out /* [n_links] or NULL */, uint64_t *any_out /* [W] or NULL */,
                       uint64_t *link_hits_out /* [n_links * W] or NULL */, uint64_t *counts_out /* [n_pat] or NULL */, kmpgpu_timing *t);

/* Fill a device arena with the synthetic payloads of kmp_synth.h (benchmark input S1/S2):
 * packet ids first_pkt_id .. first_pkt_id + n_pkts - 1 at the slots of the given device index. */
int  kmpgpu_synth_fill(kmpgpu_ctx *ctx, void *d_arena, const void *d_pkt_off, const void *d_pkt_len,
                       uint64_t first_pkt_id, uint64_t n_pkts, const kmp_synth_params *sp);

/* Device-side index for n fixed-length payloads at stride round_up(len, align): writes
 * d_pkt_off[k] = k * stride, d_pkt_len[k] = len. */
int  kmpgpu_fixed_index(kmpgpu_ctx *ctx, void *d_pkt_off, void *d_pkt_len, uint64_t n_pkts,
                        uint32_t len, uint32_t slot_align);

/* What the arena currently attached/loaded holds. */
int  kmpgpu_arena_info(kmpgpu_ctx *ctx, uint64_t *n_pkts, uint64_t *payload_bytes);
/* Sum over payloads of min(len, first 0x00 + 1): the bytes a strlen()-bounded scan (serial.c:191) has to
 * touch; equals payload_bytes on NUL-free input.  Reported beside the payload bytes for inputs that carry
 * NUL bytes; one extra pass over the arena, not part of kmpgpu_scan.  Always the strlen figure, whatever
 * KMPGPU_OPT_WHOLE_PAYLOAD says: a whole-payload pass looks at all payload_bytes (kmpgpu_arena_info). */
int  kmpgpu_effective_bytes(kmpgpu_ctx *ctx, uint64_t *bytes_out);
/* Copy the context's device arena + index back to host buffers (tests: the on-device extraction must
 * build exactly the arena the host builds).  Buffers sized from kmpgpu_arena_info / arena_bytes. */
int  kmpgpu_arena_download(kmpgpu_ctx *ctx, uint8_t *arena_out, uint64_t arena_cap, uint64_t *arena_bytes,
                           uint64_t *pkt_off_out, uint32_t *pkt_len_out);

#ifdef __cplusplus
}
#endif
#endif /* KMPGPU_H */
