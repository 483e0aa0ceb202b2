/* kmp_launch.h -- launch entry points of kmp_scan_*.hip / kmp_prep.hip / kmp_fold.hip / kmp_marks.hip / kmp_rules.hip / kmp_relations.hip /
 * kmp_chains.hip / kmp_headers.hip / kmp_bytetests.hip / kmp_regex.hip / kmp_links.hip / kmp_select.hip / kmp_decode.hip / kmp_base64.hip / kmp_fields.hip / kmp_dns.hip / kmp_tls.hip / kmp_alerts.hip / kmp_flows.hip / kmp_seams.hip / kmp_streams.hip / kmp_streams_seq.hip / kmp_flowbits.hip / kmp_thresholds.hip, used
 * by the C-ABI layer (kmpgpu.hip), which alone decides what is launched; the tables kmp_launch_scan_multi takes come from kmp_tables.h. */
#ifndef KMP_LAUNCH_H
#define KMP_LAUNCH_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kmp_device.h"

struct kmp_scan_args {
    const uint8_t         *arena;
    const uint64_t        *pkt_off;
    const uint32_t        *pkt_len;
    uint64_t               n_pkts;
    const kmp_pattern_dev *patterns;     /* all patterns, file order                         */
    const uint32_t        *pat_ids;      /* pattern index handled by blockIdx.y              */
    uint32_t               n_ids;        /* gridDim.y                                        */
    unsigned long long    *partials;     /* [n_ids][blocks_x]                                */
    unsigned long long    *zero_counts;  /* flat / packed kernels: counts[] to put to 0 for the patterns of this launch (sliced reduce without accumulation), or NULL */
    uint32_t               blocks_x;
    int                    depth;        /* chunk loads in flight per wavefront              */
    int                    mode;         /* 0 filter + confirm, 1 automaton only             */
    bool                   masked;       /* every pattern of this launch is shorter than 4   */
    bool                   nontemporal;
    bool                   whole;        /* KMPGPU_OPT_WHOLE_PAYLOAD: E_k = L_k, the whole-payload instantiations */
    /* flat kernel only: every payload has length uniform_len, payload k starts at arena + k * uniform_stride */
    uint32_t               uniform_stride;
    uint32_t               uniform_len;
    uint32_t               pkts_per_wave;
    /* packed kernel only */
    const unsigned long long *bitmap;   /* one bit per 16-byte slot of the arena: a payload starts here */
    const void            *plan;         /* kmp_plan_entry[waves + 1]; fused pass: [units + 1]          */
    /* fused pass only: the arena in `fused_blocks` regions of `units_per_block` work units each (kmp_plan_shape) */
    uint32_t               fused_blocks, units_per_block, n_units;   /* units_per_block: per REGION, which fused_sides (1 or 2) blocks share */
    uint32_t               fused_sides;
    bool                   fused_classed; /* the group of this launch is a classed one (kmp_device.h): cshift is a shift; a plain group: its short patterns */
    uint32_t              *fused_pool;   /* [regions] next unit of the region's pool, all 0 before the launch */
    uint64_t               span_end;     /* end of the last slot                                        */
    bool                   pad_clean;    /* every byte between a payload's end and the next slot is 0x00 */
    /* match-offset emission (streaming kernels only): kmpgpu_match[emit_cap], running counter */
    void                  *emit_out;
    unsigned long long    *emit_counter;
    unsigned long long     emit_cap;
    /* hit-matrix marking (kmpgpu_scan_packets): bit k of row i of emit_marks[mark_rows][mark_stride] is set where payload k
     * holds pattern i.  Runs the same EMIT kernels, grid and plan as the offsets pass, writing no record */
    unsigned long long    *emit_marks;
    uint32_t               mark_stride, mark_rows;
    /* per-pattern offset windows (kmpgpu_set_windows): {first, last} by pattern index, 8 bytes each; a match is reported or marked only
     * where first <= its offset in the payload <= last.  Set only for a pass that emits or marks, NULL where no window differs from the
     * default [0, UINT32_MAX] */
    const void            *emit_windows;
};

/* the pass writes offset records or marks: the launchers take the EMIT instantiations */
static inline bool kmp_emits(const kmp_scan_args &a) { return a.emit_out != nullptr || a.emit_marks != nullptr; }

hipError_t kmp_launch_scan(const kmp_scan_args &a, hipStream_t st);
hipError_t kmp_launch_scan_flat(const kmp_scan_args &a, hipStream_t st);
hipError_t kmp_launch_scan_packed(const kmp_scan_args &a, hipStream_t st);
hipError_t kmp_launch_build_bitmap(const uint64_t *pkt_off, uint64_t n, unsigned long long *bitmap, hipStream_t st);
/* Where the ranges of a plan are cut (before the closest packet start is taken).  units == 0: entry w at w * step bytes from the first
 * packet.  Otherwise the arena goes in regions of `region` bytes, one per block of the fused pass, and every region in `units` work
 * units: `big_units` of `step` bytes, then (the last part of a region, taken when its block is about to run out of work) units of `small`. */
struct kmp_plan_shape { uint64_t step; uint64_t region; uint32_t units, big_units, small; };
hipError_t kmp_launch_plan(const uint64_t *pkt_off, const uint32_t *pkt_len, uint64_t n, uint64_t nwaves, const kmp_plan_shape &shape,
                           void *plan, hipStream_t st);
hipError_t kmp_launch_reduce(const unsigned long long *partials, uint32_t blocks_x, const uint32_t *pat_ids,
                             uint32_t n_ids, unsigned long long *counts, hipStream_t st, const uint32_t *rows = nullptr,
                             int accumulate = 0, bool counts_zeroed = false);
#define KMP_REDUCE_SLICE 4096u            /* partials one block of kmp_reduce_kernel adds up */
/* more than 16384 partials per pattern are summed by several blocks that ADD to counts[]: the scan kernel zeroes it first (zero_counts) */
static inline bool kmp_reduce_is_sliced(uint32_t blocks_x) { return blocks_x > 16384u; }
hipError_t kmp_launch_scan_multi(const kmp_scan_args &a, const uint32_t *tables, uint32_t table_words, uint32_t n_unique, uint32_t cshift, uint32_t bucket_mask, uint32_t n_ones, uint32_t ones,
                                 const uint32_t *uid_first, const uint32_t *uid_ids, hipStream_t st);
size_t kmp_multi_lds_bytes(uint32_t table_words, uint32_t n_unique, uint32_t waves);
int kmp_multi_kind(bool emit, bool pad_clean, uint32_t n_ones);
uint32_t kmp_multi_block_waves(int kind);
uint32_t kmp_multi_resident_waves(int kind, uint32_t table_words, uint32_t n_unique);
#define KMP_SCAN_ITEMS 4u                                         /* items per thread in the block scan of kmp_prep.hip */
#define KMP_SCAN_TILE  (KMP_BLOCK_THREADS * KMP_SCAN_ITEMS)      /* items per block: the scan workspace holds one total per tile */
size_t kmp_extract_ws_bytes(uint64_t n_frames);
/* The scan workspace, kmp_extract_ws_bytes(n) bytes, and the one place that spells its layout: loc_off[n], blk_bytes[nblk], then the 32-bit
 * arrays aux[n], len[n], loc_idx[n], blk_cnt[nblk], with nblk tiles of KMP_SCAN_TILE items.  len[i] is the length of item i in the
 * destination, or 0xFFFFFFFF ("not in dst"); the scan (kmp_launch_compact_scan) leaves item i at byte blk_bytes[i / KMP_SCAN_TILE] +
 * loc_off[i] of a packed arena, as payload blk_cnt[i / KMP_SCAN_TILE] + loc_idx[i].  aux is the caller's and the scan does not touch it:
 * the extractor's payload offsets, the seams' pred[]. */
struct kmp_compact_view {
    uint64_t *loc_off, *blk_bytes;
    uint32_t *aux, *len, *loc_idx, *blk_cnt;
    uint32_t  nblk;
};
static inline kmp_compact_view kmp_compact_ws(uint8_t *ws, uint64_t n)
{
    kmp_compact_view w;
    w.nblk = (uint32_t)((n + KMP_SCAN_TILE - 1) / KMP_SCAN_TILE);
    w.loc_off = reinterpret_cast<uint64_t *>(ws);
    w.blk_bytes = w.loc_off + n;
    w.aux = reinterpret_cast<uint32_t *>(w.blk_bytes + w.nblk);
    w.len = w.aux + n;
    w.loc_idx = w.len + n;
    w.blk_cnt = w.loc_idx + n;
    return w;
}
/* kmp_scan_local_kernel + kmp_scan_totals_kernel over the len[] of such a workspace: totals[0] = bytes of the packed result, totals[1] =
 * its items.  What every compacting builder runs between its lengths and its index kernel. */
hipError_t kmp_launch_compact_scan(uint64_t n, uint8_t *ws, unsigned long long *totals, hipStream_t st);

/* The grids of the compacting builders ("The compacting skeleton"), all capped at KMP_GRID_CAP blocks and grid-stride beyond:
 * a thread per item, a wavefront per group of 64 items, and a wavefront per RUN of consecutive destination payloads.  A run is a power
 * of two up to 64 payloads that brings `bytes / n_dst`, the average payload, to KMP_RUN_BYTES. */
#define KMP_GRID_CAP  1024u
#define KMP_RUN_BYTES 16384u
static inline uint32_t kmp_grid_cap(uint64_t blocks) { return (uint32_t)(blocks < KMP_GRID_CAP ? blocks : KMP_GRID_CAP); }
static inline uint32_t kmp_item_blocks(uint64_t n) { return kmp_grid_cap((n + KMP_BLOCK_THREADS - 1) / KMP_BLOCK_THREADS); }
static inline uint32_t kmp_group_blocks(uint64_t n) { return kmp_grid_cap(((n + KMP_WAVE - 1) / KMP_WAVE + KMP_BLOCK_WAVES - 1) / KMP_BLOCK_WAVES); }
struct kmp_run_shape { uint32_t run, blocks; };
static inline kmp_run_shape kmp_run_shape_of(uint64_t n_dst, uint64_t bytes)
{
    const uint64_t avg = bytes / n_dst > 16 ? bytes / n_dst : 16;
    kmp_run_shape s;
    s.run = KMP_WAVE;
    while (s.run > 1u && (uint64_t)s.run * avg > KMP_RUN_BYTES) s.run >>= 1;
    s.blocks = kmp_grid_cap(((n_dst + s.run - 1) / s.run + KMP_BLOCK_WAVES - 1) / KMP_BLOCK_WAVES);
    return s;
}
hipError_t kmp_launch_extract_phase1(const uint8_t *file, const uint64_t *frame_off, const uint32_t *caplen, uint64_t n, int tcp,
                                     uint8_t *ws, unsigned long long *totals, hipStream_t st);
hipError_t kmp_launch_extract_phase2(const uint8_t *file, const uint64_t *frame_off, uint64_t n, uint8_t *ws, uint64_t n_pkts,
                                     uint8_t *arena, uint64_t *pkt_off, uint32_t *pkt_len, uint64_t *src_off, hipStream_t st);
hipError_t kmp_launch_repack_phase1(const uint32_t *pkt_len, uint64_t n, uint8_t *ws, unsigned long long *totals, hipStream_t st);
hipError_t kmp_launch_repack_phase2(const uint8_t *old_arena, const uint64_t *old_off, const uint32_t *pkt_len, uint64_t n, uint8_t *ws,
                                    uint8_t *new_arena, uint64_t *new_off, hipStream_t st);
hipError_t kmp_launch_check_padding(uint8_t *arena, const uint64_t *pkt_off, const uint32_t *pkt_len, uint64_t n, int fix,
                                    uint32_t *dirty, hipStream_t st);
hipError_t kmp_launch_effective_bytes(const uint8_t *arena, const uint64_t *pkt_off, const uint32_t *pkt_len, uint64_t n,
                                      unsigned long long *out, hipStream_t st);
hipError_t kmp_launch_validate(const uint64_t *pkt_off, const uint32_t *pkt_len, uint64_t n, uint64_t arena_bytes,
                               uint32_t *err, unsigned long long *payload_bytes, hipStream_t st);
hipError_t kmp_launch_synth_fill(uint8_t *arena, const uint64_t *pkt_off, const uint32_t *pkt_len, uint64_t first_pkt_id,
                                 uint64_t n, const kmp_synth_params &sp, hipStream_t st);
hipError_t kmp_launch_add_counts(unsigned long long *dst, const unsigned long long *src, uint32_t n, hipStream_t st);
/* kmp_fold.hip: dst[0, bytes) = src[0, bytes) with ASCII A-Z lowercased (bytes a multiple of 16, both 16-byte aligned), and the end
 * of the furthest slot of an index (atomicMax into *end, which the caller zeroes) */
hipError_t kmp_launch_fold(const uint8_t *src, uint8_t *dst, uint64_t bytes, hipStream_t st);
hipError_t kmp_launch_slot_end(const uint64_t *pkt_off, const uint32_t *pkt_len, uint64_t n, unsigned long long *end, hipStream_t st);
/* kmp_marks.hip: per row of the hit matrix marks[n_rows][stride] (stride even, the matrix 16-byte aligned) the number of set bits,
 * added to pkt_counts[row], and per column word the OR over all rows, ORed into any[word]; both zeroed by the caller */
hipError_t kmp_launch_marks_reduce(const unsigned long long *marks, uint32_t n_rows, uint64_t stride, unsigned long long *pkt_counts,
                                   unsigned long long *any, hipStream_t st);
/* kmp_rules.hip: the rules of kmpgpu_set_rules over the hit matrix marks[n_pat][stride] (stride even, 16-byte aligned) that holds n_pkts
 * payloads.  The rules lie on the device as CSR in 16-byte units.  A term is a pattern index (< n_pat, checked by the caller) |
 * KMPGPU_RULE_NOT (kmpgpu.h) for a negated term.  heads[r] = {first quad of rule r's further terms, the quad behind its last, its first term, its
 * second term}, quads[q] = four further terms; a rule of one term has it twice in its head, and the last quad of a rule is filled up
 * with repeats of that quad's first term (a repeated term changes nothing, and no load of the kernel hangs on a condition).  Every word of
 * rule_rows[n_rules][stride] is written (the bits of index n_pkts and above as 0), a rule's set bits are added to rule_counts[r],
 * the OR over all rules is ORed into any[stride]; the caller zeroes those two */
hipError_t kmp_launch_rules(const unsigned long long *marks, uint64_t stride, uint64_t n_pkts, const uint4 *heads, const uint4 *quads,
                            uint32_t n_rules, unsigned long long *rule_rows, unsigned long long *rule_counts, unsigned long long *any,
                            hipStream_t st);
/* kmp_relations.hip: the relations of kmpgpu_set_relations, decided for the payloads that hold both patterns.  marks[..][stride] is the hit
 * matrix the marking pass has just filled for n_pkts payloads (rows = pattern indices); relations[q] = {a | A << 31, b | B << 31, dmin,
 * dmax} with a, b < 2^31 pattern indices (checked by the caller) and A / B set where that pattern's bytes are compared in `fold`, the
 * folded copy of the arena (a pattern of the nocase set; patterns[i].pat is folded then), instead of `arena`.  windows: {first, last} per
 * pattern index or NULL; whole: E_k = L_k.  Word j < ceil(n_pkts / 64) of rows[q][stride] is written for every q (the caller zeroes the
 * padding word of an odd row), a relation's set bits are added to rel_counts[q] and ORed into any[]; the caller zeroes those two.  At most
 * max_blocks blocks, grid-stride. */
hipError_t kmp_launch_relations(const unsigned long long *marks, uint64_t stride, uint64_t n_pkts, const uint4 *relations, uint32_t n_rel,
                                const kmp_pattern_dev *patterns, const uint8_t *arena, const uint8_t *fold, const uint64_t *pkt_off,
                                const uint32_t *pkt_len, const void *windows, bool whole, uint32_t max_blocks, unsigned long long *rows,
                                unsigned long long *rel_counts, unsigned long long *any, hipStream_t st);
/* kmp_chains.hip: the chains of kmpgpu_set_chains, decided for the payloads that hold every content.  As kmp_launch_relations, but for
 * chains[c * KMPGPU_CHAIN_MAX + i] = {p_i | F << 31, dmin_i, dmax_i, n}: link i < n of chain c (2 <= n <= KMPGPU_CHAIN_MAX, checked by the
 * caller; the bounds of link 0 are not read, the records behind link n - 1 neither), F set where that pattern's bytes are compared in
 * `fold`.  Word j < ceil(n_pkts / 64) of rows[c][stride] is written for every c, a chain's set bits are added to chain_counts[c] and ORed
 * into any[]; the caller zeroes those two.  At most max_blocks blocks, grid-stride. */
hipError_t kmp_launch_chains(const unsigned long long *marks, uint64_t stride, uint64_t n_pkts, const uint4 *chains, uint32_t n_chains,
                             const kmp_pattern_dev *patterns, const uint8_t *arena, const uint8_t *fold, const uint64_t *pkt_off,
                             const uint32_t *pkt_len, const void *windows, bool whole, uint32_t max_blocks, unsigned long long *rows,
                             unsigned long long *chain_counts, unsigned long long *any, hipStream_t st);
/* kmp_headers.hip: the header predicates of kmpgpu_set_headers, decided from meta[n_pkts] (16-byte kmpgpu_pkt_meta records, 16-byte
 * aligned) and pkt_len[n_pkts] alone.  preds[q * 3 ..]: the 48-byte record of predicate q as kmp_pack_headers leaves it (kmp_rowtables.h),
 * taken KMP_HDR_TILE at a time.  Every word of rows[q][stride] (stride even, 16-byte aligned) is written for every q, the bits of index
 * n_pkts and above as 0; a predicate's set bits are added to hdr_counts[q] and ORed into any[]; the caller zeroes those two. */
#define KMP_HDR_TILE 128u
hipError_t kmp_launch_headers(const void *meta, const uint32_t *pkt_len, uint64_t n_pkts, uint64_t stride, const uint4 *preds,
                              uint32_t n_hdr, unsigned long long *rows, unsigned long long *hdr_counts, unsigned long long *any,
                              hipStream_t st);
/* kmp_bytetests.hip: the byte tests of kmpgpu_set_bytetests.  tests[q * 2 ..]: the 32-byte record of test q as kmp_pack_bytetests leaves
 * it (kmp_rowtables.h), rel_idx[n_relative]: the indices of the relative tests, ascending.  One kernel per call.  relative = false: the
 * absolute tests (none: no launch), taken KMP_BT_TILE records at a time, from arena / pkt_off / pkt_len alone; H: the largest offset +
 * nbytes among them; every word of their rows[q][stride] (stride even, 16-byte aligned) is written, the bits of index n_pkts and above as
 * 0.  relative = true: the relative tests (none: no launch), as kmp_launch_relations: candidates from marks[anchor][stride], word
 * j < ceil(n_pkts / 64) of their rows written, at most max_blocks blocks, grid-stride.  Either kernel writes its own rows only, adds a
 * test's set bits to bt_counts[q] and ORs them into any[]; the caller zeroes those two.  Field bytes come from `arena`, never from `fold`. */
#define KMP_BT_TILE 128u
hipError_t kmp_launch_bytetests(bool relative, const unsigned long long *marks, uint64_t stride, uint64_t n_pkts, const uint4 *tests,
                                uint32_t n_bt, const uint32_t *rel_idx, uint32_t n_relative, uint32_t H, const kmp_pattern_dev *patterns,
                                const uint8_t *arena, const uint8_t *fold, const uint64_t *pkt_off, const uint32_t *pkt_len,
                                const void *windows, bool whole, uint32_t max_blocks, unsigned long long *rows,
                                unsigned long long *bt_counts, unsigned long long *any, hipStream_t st);
/* kmp_regex.hip: the expressions of kmpgpu_set_regexes.  tables: the tiles of KMP_RX_TILE expressions as kmp_pack_regexes leaves them
 * (kmp_regex.h, kmp_rowtables.h).  One kernel per call, from arena / pkt_off / pkt_len and, for the gated expressions, the gate patterns'
 * rows of marks[][stride] alone; text ends at the first 0x00, or at pkt_len with whole.  Every word of rows[q][stride] (stride even, 16-byte
 * aligned) is written, the bits of index n_pkts and above as 0; an expression's set bits are added to rx_counts[q] and ORed into any[]; the
 * caller zeroes those two.  No other family's row is written. */
hipError_t kmp_launch_regexes(const unsigned long long *marks, uint64_t stride, uint64_t n_pkts, const uint4 *tables, uint32_t n_rx,
                              const uint8_t *arena, const uint64_t *pkt_off, const uint32_t *pkt_len, bool whole,
                              unsigned long long *rows, unsigned long long *rx_counts, unsigned long long *any, hipStream_t st);
/* kmp_regex_groups.hip: the expressions under KMPGPU_RX_GROUPS, behind kmp_launch_regexes with its arguments.  tables: the tiles of
 * KMP_RXG_TILE expressions as kmp_pack_regex_groups leaves them, n_groups of them; each writes every word of the row rows[q][stride] its
 * record names, adds to rx_counts[q] and ORs into any[].  No other row is written. */
hipError_t kmp_launch_regex_groups(const unsigned long long *marks, uint64_t stride, uint64_t n_pkts, const uint4 *tables, uint32_t n_groups,
                                   const uint8_t *arena, const uint64_t *pkt_off, const uint32_t *pkt_len, bool whole,
                                   unsigned long long *rows, unsigned long long *rx_counts, unsigned long long *any, hipStream_t st);
/* kmp_links.hip (kmpgpu_link_rows): rows of another context's matrix in this one's payload numbering (the definition: kmpgpu.h).
 * _rank (2 kernels; KMPGPU_LINK_BITMAP only): over bitmap[ceil(n_dst / 64)], bits at n_dst and above not counted, into ws
 *   (kmp_link_rank_bytes(n_dst) bytes, 8-byte aligned): tile_base[tiles + 1], 64 bits each, one per KMP_LINK_RANK_TILE map words, the last
 *   one the number of set bits below n_dst (kmp_link_rank_total), then rank[ceil(n_dst / 64)], 32 bits each, inside the word's tile.
 * _gather (1 kernel): word j < ceil(n_dst / 64) of dst_rows[r][dst_stride] for every r < n_rows: bit k = bit map(k) of src_rows[r][src_stride]
 *   where k < n_dst, map(k) exists and map(k) < n_src, else 0.  kind KMPGPU_LINK_SAME: map(k) = k, map and rank_ws not read, both strides
 *   the same even number, the rows 16-byte aligned; _BITMAP: map = the bitmap of _rank and rank_ws its ws; _INDEX: map = uint32_t[n_dst],
 *   rank_ws not read.  The padding word of an odd destination row is the caller's, except under _SAME, which copies whole 16-byte
 *   pairs and writes it as 0.  No word of a source row behind that of payload n_src - 1 is read -- under _SAME the padding word of an odd
 *   source row, which lies inside the row, is loaded with its pair and masked to 0 -- and no map entry at n_dst or behind.  At most KMP_GRID_CAP blocks, grid-stride. */
#define KMP_LINK_RANK_TILE 1024u
size_t kmp_link_rank_bytes(uint64_t n_dst);
static inline const unsigned long long *kmp_link_rank_total(const uint8_t *ws, uint64_t n_dst)
{
    return reinterpret_cast<const unsigned long long *>(ws) + ((n_dst + 63u) / 64u + KMP_LINK_RANK_TILE - 1u) / KMP_LINK_RANK_TILE;
}
hipError_t kmp_launch_link_rank(const unsigned long long *bitmap, uint64_t n_dst, uint8_t *ws, hipStream_t st);
hipError_t kmp_launch_link_gather(int kind, const unsigned long long *src_rows, uint64_t src_stride, uint64_t n_src, uint32_t n_rows,
                                  uint64_t n_dst, const void *map, const uint8_t *rank_ws, unsigned long long *dst_rows,
                                  uint64_t dst_stride, hipStream_t st);
/* ... and the metadata itself.  _extract: behind kmp_launch_extract_phase2, with its arguments and its workspace: meta[k] of every accepted
 * frame, k as kmp_scatter_index_kernel numbers the payloads.  _select: behind kmp_launch_select_phase2, with the workspace of the selection
 * over src's n payloads: meta[j] = src_meta[k] for the j-th selected payload k.  One kernel each. */
hipError_t kmp_launch_meta_extract(const uint8_t *file, const uint64_t *frame_off, uint64_t n, const uint8_t *ws, void *meta, hipStream_t st);
hipError_t kmp_launch_meta_select(const void *src_meta, uint64_t n, const uint8_t *ws, void *meta, hipStream_t st);
hipError_t kmp_launch_fixed_index(uint64_t *pkt_off, uint32_t *pkt_len, uint64_t n, uint32_t len, uint64_t stride,
                                  hipStream_t st);
/* kmp_select.hip (kmpgpu_load_selected): the payloads of an index of n whose bit is set in select[ceil(n / 64)] (payload k: bit k & 63 of
 * word k >> 6; bits at n and above are not read as payloads), compacted into a packed arena.  The compacting builders -- this one,
 * kmp_decode.hip, kmp_base64.hip, kmp_fields.hip, kmp_seams.hip -- have these in common: ws is the scan workspace above, kept from the
 * lengths to the index; between those two runs kmp_launch_compact_scan, which leaves totals[0] = total_bytes and totals[1] = n_dst;
 * the index writes pkt_off[n_dst], pkt_len[n_dst] and the 16-byte records recs[n_dst] the last kernel reads; that one writes
 * arena[0, total_bytes), every slot whole and 0x00 behind its payload's end; the source's slots are 16-byte aligned (the layout
 * contract of kmpgpu.h), of src_arena only aligned 16-byte units that hold a byte of a payload are read, and nothing at or behind a
 * payload's end takes part.  Here: phase 1 (3 kernels) is the lengths and the scan, phase 2 (2 kernels) the index and the copy. */
hipError_t kmp_launch_select_phase1(const unsigned long long *select, const uint32_t *pkt_len, uint64_t n, uint8_t *ws,
                                    unsigned long long *totals, hipStream_t st);
hipError_t kmp_launch_select_phase2(const uint8_t *src_arena, const uint64_t *src_off, uint64_t n, uint8_t *ws, uint64_t n_sel,
                                    uint64_t total_bytes, uint8_t *arena, uint64_t *pkt_off, uint32_t *pkt_len, void *recs,
                                    bool nontemporal, hipStream_t st);
/* kmp_decode.hip (kmpgpu_load_decoded): the n payloads of an index percent-decoded (the definition: kmpgpu.h) into a packed arena, ws
 * as kmp_select.hip's.  _lengths (1 kernel) leaves per payload its decoded length, or 0xFFFFFFFF for an unchanged one with only_changed,
 * writes every word of changed[ceil(n / 64)] (bits at n and above 0) and adds to stats[3] = {source bytes of the payloads kept, changed
 * payloads, decoded bytes}, which the caller zeroes.  Then kmp_launch_compact_scan (2 kernels), _index (1 kernel) and _write (1 kernel).
 * bytes_in: stats[0]. */
hipError_t kmp_launch_decode_lengths(const uint8_t *src_arena, const uint64_t *src_off, const uint32_t *src_len, uint64_t n, bool plus,
                                     bool only_changed, uint8_t *ws, unsigned long long *changed, unsigned long long *stats, hipStream_t st);
hipError_t kmp_launch_decode_index(const uint64_t *src_off, const uint32_t *src_len, uint64_t n, uint8_t *ws, uint64_t n_dst, uint64_t *pkt_off,
                                   uint32_t *pkt_len, void *recs, hipStream_t st);
hipError_t kmp_launch_decode_write(const uint8_t *src_arena, const uint64_t *pkt_off, const void *recs, uint64_t n_dst, uint64_t bytes_in,
                                   uint64_t total_bytes, bool plus, uint8_t *arena, bool nontemporal, hipStream_t st);
/* kmp_base64.hip (kmpgpu_load_base64): the base64 runs of min_run (4..255) alphabet bytes and more decoded (the definition: kmpgpu.h).
 * The phases, ws, changed, stats and recs are those of kmp_decode.hip: _lengths (1 kernel) and _write (1 kernel) here, and between
 * them kmp_launch_compact_scan and kmp_launch_decode_index, whose records these two share. */
hipError_t kmp_launch_base64_lengths(const uint8_t *src_arena, const uint64_t *src_off, const uint32_t *src_len, uint64_t n, uint32_t min_run,
                                     bool urlsafe, bool only_changed, uint8_t *ws, unsigned long long *changed, unsigned long long *stats,
                                     hipStream_t st);
hipError_t kmp_launch_base64_write(const uint8_t *src_arena, const uint64_t *pkt_off, const void *recs, uint64_t n_dst, uint64_t bytes_in,
                                   uint64_t total_bytes, uint32_t min_run, bool urlsafe, uint8_t *arena, bool nontemporal, hipStream_t st);
/* kmp_fields.hip (kmpgpu_http_locate, kmpgpu_load_fields): the HTTP field buffers (the definition: kmpgpu.h).  _http_locate (1 kernel)
 * writes spans[n] (kmpgpu_http_span, 32 bytes each, 16-byte aligned) and adds to stats[4] = {requests, responses, messages with a blank
 * line, bytes scanned}, which the caller zeroes.  The rest as kmp_select.hip's: _lengths (1 kernel) leaves per payload the length of
 * `field` (KMPGPU_FIELD_*), or 0xFFFFFFFF for an absent one with only_present, writes every word of present[ceil(n / 64)] (bits at n and
 * above 0) and adds to stats[3] = {source bytes of the payloads kept, payloads with the field, field bytes}, which the caller zeroes.
 * Then kmp_launch_compact_scan (2 kernels), _index (1 kernel) and _gather (1 kernel). */
hipError_t kmp_launch_http_locate(const uint8_t *src_arena, const uint64_t *src_off, const uint32_t *src_len, uint64_t n, void *spans,
                                  unsigned long long *stats, hipStream_t st);
hipError_t kmp_launch_fields_lengths(const void *spans, const uint32_t *src_len, uint64_t n, int field, bool only_present, uint8_t *ws,
                                     unsigned long long *present, unsigned long long *stats, hipStream_t st);
hipError_t kmp_launch_fields_index(const void *spans, const uint64_t *src_off, uint64_t n, int field, uint8_t *ws, uint64_t n_dst,
                                   uint64_t *pkt_off, uint32_t *pkt_len, void *recs, hipStream_t st);
hipError_t kmp_launch_fields_gather(const uint8_t *src_arena, const uint64_t *pkt_off, const void *recs, uint64_t n_dst, uint64_t total_bytes,
                                    uint8_t *arena, bool nontemporal, hipStream_t st);
/* kmp_dns.hip (kmpgpu_dns_locate, kmpgpu_load_dns): the DNS query-name buffers (the definition: kmpgpu.h).  _dns_locate (1 kernel) writes
 * spans[n] (kmpgpu_dns_span, 32 bytes each, 16-byte aligned) and masks[n] (32 bytes each: bit x set where byte x of payload k's name is a
 * label's length byte, all zero for a payload that is no message) and adds to stats[4] = {queries, responses, root names, name bytes},
 * which the caller zeroes.  The rest as kmp_fields.hip's, with the name as the one field and the masks read by the gather. */
hipError_t kmp_launch_dns_locate(const uint8_t *src_arena, const uint64_t *src_off, const uint32_t *src_len, uint64_t n, bool tcp_prefix,
                                 void *spans, void *masks, unsigned long long *stats, hipStream_t st);
hipError_t kmp_launch_dns_lengths(const void *spans, const uint32_t *src_len, uint64_t n, bool only_present, uint8_t *ws,
                                  unsigned long long *present, unsigned long long *stats, hipStream_t st);
hipError_t kmp_launch_dns_index(const void *spans, const uint64_t *src_off, uint64_t n, uint8_t *ws, uint64_t n_dst, uint64_t *pkt_off,
                                uint32_t *pkt_len, void *recs, hipStream_t st);
hipError_t kmp_launch_dns_gather(const uint8_t *src_arena, const uint64_t *pkt_off, const void *recs, const void *masks, uint64_t n_dst,
                                 uint64_t total_bytes, uint8_t *arena, bool nontemporal, hipStream_t st);
/* kmp_tls.hip (kmpgpu_tls_locate, kmpgpu_load_tls): the TLS ClientHello buffers (the definition: kmpgpu.h).  _tls_locate (1 kernel) writes
 * spans[n] (kmpgpu_tls_span, 32 bytes each, 16-byte aligned) and masks[n] (32 bytes each: bit x set where byte x of payload k's ALPN field
 * is a name's length byte, all zero for a payload without the field) and adds to stats[4] = {hellos, with a server name, with an ALPN
 * field, truncated}, which the caller zeroes.  The rest as kmp_dns.hip's, with `field` KMPGPU_TLS_SNI or KMPGPU_TLS_ALPN; the gather reads
 * the masks for KMPGPU_TLS_ALPN only. */
hipError_t kmp_launch_tls_locate(const uint8_t *src_arena, const uint64_t *src_off, const uint32_t *src_len, uint64_t n, void *spans,
                                 void *masks, unsigned long long *stats, hipStream_t st);
hipError_t kmp_launch_tls_lengths(const void *spans, const uint32_t *src_len, uint64_t n, int field, bool only_present, uint8_t *ws,
                                  unsigned long long *present, unsigned long long *stats, hipStream_t st);
hipError_t kmp_launch_tls_index(const void *spans, const uint64_t *src_off, uint64_t n, int field, uint8_t *ws, uint64_t n_dst,
                                uint64_t *pkt_off, uint32_t *pkt_len, void *recs, hipStream_t st);
hipError_t kmp_launch_tls_gather(const uint8_t *src_arena, const uint64_t *pkt_off, const void *recs, const void *masks, int field,
                                 uint64_t n_dst, uint64_t total_bytes, uint8_t *arena, bool nontemporal, hipStream_t st);
/* kmp_alerts.hip (kmpgpu_scan_alerts): the set bits of rows[n_rows][stride] (stride even, 16-byte aligned, every word of a row readable,
 * the bits of index n_pkts and above not looked at; 16 * n_rows <= 0xFFFFFFFE) as 16-byte records {payload (64 bits), row, 0}, sorted by
 * payload, then row.  any[ceil(n_pkts / 64)]: the OR over the rows, complete before the count; a column word whose any word is 0 is not read.
 * ws: kmp_extract_ws_bytes(n_pkts) bytes, kept from the count to the fill.  _count (1 kernel) leaves per payload its records' bytes, kmp_launch_compact_scan
 * (2 kernels) every payload's offset and totals[0] = 16 * records, totals[1] = payloads with a record, _fill (1 kernel) writes the records
 * whose position in the list is below max_records to recs[min(max_records, records)]. */
hipError_t kmp_launch_alerts_count(const unsigned long long *rows, uint64_t stride, uint32_t n_rows, uint64_t n_pkts,
                                   const unsigned long long *any, uint8_t *ws, hipStream_t st);
hipError_t kmp_launch_alerts_fill(const unsigned long long *rows, uint64_t stride, uint32_t n_rows, uint64_t n_pkts,
                                  const unsigned long long *any, uint8_t *ws, void *recs, uint64_t max_records, hipStream_t st);

/* kmp_flows.hip (kmpgpu_flows_build, kmpgpu_scan_flows, kmpgpu_flows_select): the n_pkts <= 2^32 - 2 payloads of meta[] (16-byte
 * kmpgpu_pkt_meta records, 16-byte aligned) grouped by their flow key (kmp_flow_key.h).  In the order they are launched:
 * _insert: table[slots] (a power of two > n_pkts, at most 2^32; all 0 before the launch) takes every key, first[slots] (all 0xFFFFFFFF
 *   before) the lowest payload index of every taken slot, slot_of[n_pkts] every payload's slot.
 * _firsts, kmp_launch_compact_scan (2 kernels): in ws, kmp_extract_ws_bytes(n_pkts) bytes kept up to _number: which payloads are their flow's first, their
 *   rank among those, totals[1] = n_flows.
 * _number: table[slot] = the id of the slot's flow; recs[n_flows] (48-byte kmpgpu_flow records, 16-byte aligned): first_packet, first, and
 *   0 in the three fields _assign adds up.
 * _assign: slot_flow[n_pkts] holds slot_of on entry and flow_of on return; n_packets, payload_bytes (of pkt_len[]), last_packet of recs.
 * _fold: out[r][f >> 6] |= 1 << (f & 63) for every set bit k < n_pkts of rows[r][stride], f = flow_of[k] < n_flows; r < n_rows,
 *   out[n_rows][stride_f] zeroed by the caller, 64 stride_f >= n_flows.  any[ceil(n_pkts / 64)] or NULL: a column word whose any word is 0 is
 *   not read.
 * _expand: bit k of pkt_bits[ceil(n_pkts / 64)] = bit flow_of[k] of flow_bits[ceil(n_flows / 64)]; every word is written, the bits of index
 *   n_pkts and above as 0. */
hipError_t kmp_launch_flows_insert(const void *meta, uint64_t n_pkts, bool directed, uint32_t *table, uint64_t slots, uint32_t *first,
                                   uint32_t *slot_of, hipStream_t st);
hipError_t kmp_launch_flows_firsts(const uint32_t *first, const uint32_t *slot_of, uint64_t n_pkts, uint8_t *ws, hipStream_t st);
hipError_t kmp_launch_flows_number(const void *meta, uint64_t n_pkts, uint8_t *ws, const uint32_t *slot_of, uint32_t *table, void *recs,
                                   hipStream_t st);
hipError_t kmp_launch_flows_assign(const uint32_t *table, uint32_t *slot_flow, const uint32_t *pkt_len, uint64_t n_pkts, void *recs,
                                   hipStream_t st);
hipError_t kmp_launch_flows_fold(const unsigned long long *rows, uint64_t stride, uint32_t n_rows, uint64_t n_pkts,
                                 const unsigned long long *any, const uint32_t *flow_of, uint64_t n_flows, unsigned long long *out,
                                 uint64_t stride_f, hipStream_t st);
hipError_t kmp_launch_flows_expand(const unsigned long long *flow_bits, const uint32_t *flow_of, uint64_t n_pkts, unsigned long long *pkt_bits,
                                   hipStream_t st);

/* kmp_seams.hip (kmpgpu_load_seams): the seams of an index of n <= 2^32 - 2 payloads whose flows are built -- meta[n], flow_of[n],
 * flow_recs[n_flows] as kmp_flows.hip leaves them --, gathered into a packed arena.  In the order they are launched:
 * _keys: (flow_of[k] << 1 | dir(k), k) for every payload, into sort_buf (kmp_seam_sort_bytes(n, n_flows) bytes, 256-byte aligned, kept up to
 *   _phase1; 0: rocPRIM refused the size query).
 * _sort: rocprim::radix_sort_pairs over the key's live bits, stable, inside sort_buf.
 * _phase1 (3 kernels): pred[] and the seam lengths in ws (kmp_extract_ws_bytes(n) bytes, kept up to _index), their scan; totals[0] = bytes of
 *   the packed seams, totals[1] = n_seams.
 * _index: pkt_off[n_seams], pkt_len[n_seams], the kmpgpu_seam records seams[n_seams], seam_flow[n_seams], meta[n_seams] (16-byte aligned),
 *   and recs[2 n_seams] (16 bytes each), which the gather reads.
 * _gather: arena[0, total_bytes): every slot whole, 0x00 behind its seam's end.  Of src_arena only aligned 16-byte units that hold a byte of a
 *   tail or a head are read (the source's slots are 16-byte aligned: the layout contract of kmpgpu.h). */
size_t kmp_seam_sort_bytes(uint64_t n, uint64_t n_flows);
hipError_t kmp_launch_seam_keys(const void *meta, const uint32_t *flow_of, const void *flow_recs, uint64_t n, uint8_t *sort_buf, hipStream_t st);
hipError_t kmp_launch_seam_sort(uint64_t n, uint64_t n_flows, uint8_t *sort_buf, size_t sort_bytes, hipStream_t st);
hipError_t kmp_launch_seam_phase1(const uint32_t *pkt_len, uint64_t n, uint32_t reach, const uint8_t *sort_buf, uint8_t *ws,
                                  unsigned long long *totals, hipStream_t st);
hipError_t kmp_launch_seam_index(const uint64_t *src_off, const uint32_t *src_len, const void *src_meta, const uint32_t *flow_of, uint64_t n,
                                 uint32_t reach, uint8_t *ws, uint64_t *pkt_off, uint32_t *pkt_len, void *seams, uint32_t *seam_flow, void *meta,
                                 void *recs, hipStream_t st);
hipError_t kmp_launch_seam_gather(const uint8_t *src_arena, const uint64_t *pkt_off, const void *recs, uint64_t n_seams, uint64_t total_bytes,
                                  uint8_t *arena, bool nontemporal, hipStream_t st);

/* kmp_streams.hip (kmpgpu_load_streams): the payloads of every (flow, direction) of such an index concatenated in capture order, cut to
 * `depth` bytes, into a packed arena.  After kmp_launch_seam_keys and kmp_launch_seam_sort, whose sort_buf is kept up to _index, in the
 * order they are launched:
 * _phase1 (2 kernels): over the sorted positions, the heads and the exclusive sum of the members' lengths, in ws (kmp_stream_ws_bytes(n)
 *   bytes, kept up to _index); totals[0] = bytes of all members, totals[1] = n_streams.
 * _records (4 kernels): where every stream starts in the sorted order, the kmpgpu_stream records recs[n_streams], meta[n_streams] (16-byte
 *   aligned), and the scan of the slot sizes through kmp_launch_repack_phase1; totals[0] = bytes of the packed streams.
 * _index: pkt_off[n_streams], pkt_len[n_streams], the kmpgpu_stream_pos entries map[n] by source payload, and pieces (24 n bytes, 16-byte
 *   aligned): per sorted position 16 bytes {source address, bytes in front of the cut, 0}, then the 8-byte destination addresses, ascending.
 * _gather: arena[0, total_bytes): every slot whole, 0x00 behind its stream's end.  Of src_arena only aligned 16-byte units that hold a byte
 *   of a member are read (the source's slots are 16-byte aligned: the layout contract of kmpgpu.h). */
size_t kmp_stream_ws_bytes(uint64_t n);
hipError_t kmp_launch_stream_phase1(const uint32_t *pkt_len, uint64_t n, const uint8_t *sort_buf, uint8_t *ws, unsigned long long *totals,
                                    hipStream_t st);
hipError_t kmp_launch_stream_records(const void *src_meta, uint64_t n, uint64_t total, uint64_t n_streams, uint32_t depth,
                                     const uint8_t *sort_buf, uint8_t *ws, void *recs, void *meta, unsigned long long *totals, hipStream_t st);
hipError_t kmp_launch_stream_index(const uint64_t *src_off, const uint32_t *src_len, uint64_t n, uint64_t total, uint64_t n_streams,
                                   const uint8_t *sort_buf, uint8_t *ws, uint64_t *pkt_off, uint32_t *pkt_len, void *map, void *pieces,
                                   hipStream_t st);
hipError_t kmp_launch_stream_gather(const uint8_t *src_arena, const void *pieces, uint64_t n, uint64_t total_bytes, uint8_t *arena,
                                    bool nontemporal, hipStream_t st);

/* kmp_streams_seq.hip (kmpgpu_load_streams_ordered): those streams with the members of every TCP stream in sequence order, bytes already
 * delivered dropped and holes closed; seq[n] is one sequence number per payload, n <= 2^30.  After kmp_launch_seam_keys,
 * kmp_launch_seam_sort and kmp_launch_stream_phase1, whose sort_buf and ws are kept up to _index, and with ws2
 * (kmp_stream_seq_ws_bytes(n, n_flows) bytes, 256-byte aligned, kept up to _index; 0: rocPRIM refused the size query), in the order they
 * are launched:
 * _order (2 kernels and the second sort): head_pos[], key2 = key << 32 | sequence offset, (key2, val) sorted stably over the bits in use.
 * _scans (4 kernels): the running maximum of the members' ends and its tile totals, then skip[] and the sums of take and of gaps.
 * _records (3 kernels): recs[n_streams] (kmpgpu_stream), orders[n_streams] (kmpgpu_stream_order), meta[n_streams], and the scan of the slot
 *   sizes through kmp_launch_repack_phase1; total = the bytes of all members (of _phase1); totals[0] = bytes of the packed streams.
 * _index: pkt_off[n_streams], pkt_len[n_streams], map[n] (kmpgpu_stream_pos) and segs[n] (kmpgpu_stream_seg) by source payload, and pieces
 *   (24 n bytes, 16-byte aligned): per ordered position {source address, take in front of the cut, skip}, then the destination addresses.
 * _gather: arena[0, total_bytes) as kmp_launch_stream_gather writes it; of src_arena only aligned 16-byte units that hold a KEPT byte. */
size_t kmp_stream_seq_ws_bytes(uint64_t n, uint64_t n_flows);
hipError_t kmp_launch_stream_seq_order(const void *src_meta, const uint32_t *seq, uint64_t n, uint64_t n_streams, uint64_t n_flows,
                                       const uint8_t *sort_buf, uint8_t *ws, uint8_t *ws2, size_t ws2_bytes, hipStream_t st);
hipError_t kmp_launch_stream_seq_scans(const uint32_t *pkt_len, uint64_t n, const uint8_t *sort_buf, uint8_t *ws, uint8_t *ws2, hipStream_t st);
hipError_t kmp_launch_stream_seq_records(const void *src_meta, const uint32_t *seq, uint64_t n, uint64_t total, uint64_t n_streams,
                                         uint32_t depth, const uint8_t *sort_buf, uint8_t *ws, uint8_t *ws2, void *recs, void *orders,
                                         void *meta, unsigned long long *totals, hipStream_t st);
hipError_t kmp_launch_stream_seq_index(const uint64_t *src_off, const uint32_t *src_len, uint64_t n, uint64_t n_streams, const uint8_t *sort_buf,
                                       uint8_t *ws, uint8_t *ws2, uint64_t *pkt_off, uint32_t *pkt_len, void *map, void *segs, void *pieces,
                                       hipStream_t st);
hipError_t kmp_launch_stream_seq_gather(const uint8_t *src_arena, const void *pieces, uint64_t n, uint64_t total_bytes, uint8_t *arena,
                                        bool nontemporal, hipStream_t st);

/* kmp_flowbits.hip (kmpgpu_scan_flowbits): the flow bits over n <= 2^32 - 2 payloads whose flows are built (flow_of[n] < n_flows) and whose
 * rule rows rule_rows[n_rules][stride] (stride even, 64 stride >= n, the bits of index n and above 0) kmp_launch_rules has written.
 * _order (the sort and 1 kernel; once per build of the flows): order_buf (kmp_flowbits_order_bytes(n, n_flows) bytes, 256-byte aligned, kept
 *   as long as the flows; 0: rocPRIM refused the size query) takes the payloads sorted stably by flow, the inverse and the head flags.
 * Per level of kmp_pack_flowbits (kmp_rowtables.h), with acting[2 n_act] the level's 32-byte records:
 * _build (1 kernel): the level's elements at their sorted positions in ws (kmp_flowbits_ws_bytes(n) bytes, 16-byte aligned), from the rule
 *   rows and before32[n], which holds the lower levels' bits.
 * _scan (1 kernel up to KMP_SCAN_TILE payloads, else 3 per level of aggregates above the payloads' + 1; *launches is added to):
 *   before32[k] |= the level's bits before payload k, flow_state[f] |= the level's bits after flow f's last payload.  The caller zeroes
 *   both before the first level.
 * _rows (1 kernel): word j < ceil(n / 64) of before_rows[b][stride] for every bit b of level_mask; the caller zeroes the rows.
 * _final (1 kernel): every word of alert_rows[n_rules][stride] from the rule rows, the before rows and tests[n_rules] (16-byte records); a
 *   rule's set bits are added to counts[r] and ORed into any[stride]; the caller zeroes those two. */
size_t kmp_flowbits_order_bytes(uint64_t n, uint64_t n_flows);
hipError_t kmp_launch_flowbits_order(const uint32_t *flow_of, uint64_t n, uint64_t n_flows, uint8_t *order_buf, size_t order_bytes, hipStream_t st);
size_t kmp_flowbits_ws_bytes(uint64_t n);
hipError_t kmp_launch_flowbits_build(const unsigned long long *rule_rows, uint64_t stride, uint64_t n, const uint4 *acting, uint32_t n_act,
                                     const uint32_t *before32, const uint8_t *order_buf, uint8_t *ws, hipStream_t st);
hipError_t kmp_launch_flowbits_scan(uint64_t n, const uint32_t *flow_of, const uint8_t *order_buf, uint8_t *ws, uint32_t *before32,
                                    uint32_t *flow_state, uint32_t *launches, hipStream_t st);
hipError_t kmp_launch_flowbits_rows(const uint32_t *before32, uint64_t n, uint32_t level_mask, uint64_t stride, unsigned long long *before_rows,
                                    hipStream_t st);
hipError_t kmp_launch_flowbits_final(const unsigned long long *rule_rows, const unsigned long long *before_rows, uint64_t stride,
                                     const uint4 *tests, uint32_t n_rules, unsigned long long *alert_rows, unsigned long long *counts,
                                     unsigned long long *any, hipStream_t st);

/* The order buffer of kmp_launch_flowbits_order as its readers see it: order[n], inv[n] (inv[order[i]] = i), the sorted keys[n] and
 * head[n + 1] (1 where the key changes at sorted position i; head[n] = 1). */
struct kmp_order_view {
    const uint32_t *order, *inv, *keys;
    const uint8_t  *head;
};
kmp_order_view kmp_flowbits_order_view(const uint8_t *order_buf, uint64_t n);

/* kmp_thresholds.hip (kmpgpu_scan_thresholds): the rate thresholds over n <= 2^32 - 2 payloads whose rule rows kmp_launch_rules has written
 * (stride even, 64 stride >= n).  Arrays a scan runs over hold kmp_thresholds_pad(n) items (whole 16-byte loads) and are 16-byte aligned;
 * agg (kmp_thresholds_agg_bytes(n) bytes) takes the tile aggregates of either scan.  *launches is added to.
 * _time (1 kernel up to KMP_SCAN_TILE payloads, else 3 per level of aggregates + 1): T[n], the caller's timestamps, becomes their running
 *   maximum, in place.
 * _keys (1 kernel): keys[k] = the source (dst: the destination) address of meta[k]: the input of kmp_launch_flowbits_order with
 *   n_flows = 2^32, which sorts by all 32 bits.
 * _tsort (1 kernel): Ts[i] = T[order[i]] of an order buffer.
 * Per threshold, with order_buf NULL for KMPGPU_THR_BY_RULE (the identity, one tracker):
 * _count (1 kernel + the scan's): C[i] = the number of set bits of rule_row at the sorted positions 0 .. i.
 * _pass (1 kernel): word j < ceil(n / 64) of pass_row: bit k = the threshold's comparison on n[q][k] (a payload without a base hit: 0 unless
 *   window_counts is given); window_counts[n] (or NULL) takes n[q][k] for every k.  Ts: T in the track's order (T itself for BY_RULE);
 *   not read where window is KMPGPU_THR_NO_WINDOW.  The caller zeroes the row.
 * _final (1 kernel): every word of alert_rows[n_rules][stride] = the rule row AND the pass rows [n_thr][stride] the table
 *   (kmp_pack_thresholds, kmp_rowtables.h) names for the rule; a rule's set bits are added to counts[r] and ORed into any[stride]; the caller
 *   zeroes those two. */
uint64_t kmp_thresholds_pad(uint64_t n);
size_t kmp_thresholds_agg_bytes(uint64_t n);
hipError_t kmp_launch_thresholds_time(unsigned long long *T, uint64_t n, uint8_t *agg, uint32_t *launches, hipStream_t st);
hipError_t kmp_launch_thresholds_keys(const uint4 *meta, uint64_t n, bool dst, uint32_t *keys, hipStream_t st);
hipError_t kmp_launch_thresholds_tsort(const unsigned long long *T, const uint8_t *order_buf, uint64_t n, unsigned long long *Ts, hipStream_t st);
hipError_t kmp_launch_thresholds_count(const unsigned long long *rule_row, uint64_t n, const uint8_t *order_buf, uint32_t *C, uint8_t *agg,
                                       uint32_t *launches, hipStream_t st);
hipError_t kmp_launch_thresholds_pass(const unsigned long long *rule_row, uint64_t n, const uint8_t *order_buf, const unsigned long long *Ts,
                                      const uint32_t *C, uint32_t type, uint32_t count, unsigned long long window,
                                      unsigned long long *pass_row, uint32_t *window_counts, hipStream_t st);
hipError_t kmp_launch_thresholds_final(const unsigned long long *rule_rows, const unsigned long long *pass_rows, uint64_t stride,
                                       const uint32_t *table, uint32_t n_rules, unsigned long long *alert_rows, unsigned long long *counts,
                                       unsigned long long *any, hipStream_t st);

#endif
