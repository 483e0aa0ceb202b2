/*
 * kmpgpu.hip -- C-ABI layer over the gfx950 kernels (include/kmpgpu.h).  Host code only; the
 * kernels live in kmp_scan_*.hip / kmp_prep.hip.  Replaces the state the reference keeps in main()'s locals
 * (array_of_strings / prefix_array / array_of_payloads / string_count, serial.c:54,99,101,148)
 * and the hot loop serial.c:153-155.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <map>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include <dlfcn.h>
#include <unistd.h>
#include <rccl/rccl.h>          /* types and enums only: the library itself is opened with dlopen (kmpgpu_comm_*) */

#include "kmpgpu.h"
#include "kmp_device.h"
#include "kmp_flow_key.h"
#include "kmp_launch.h"
#include "kmp_rowtables.h"
#include "kmp_tables.h"

namespace {

thread_local std::string g_err;

std::atomic<uint64_t> g_ctx_ids{0};               /* kmpgpu_ctx::id */

int fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIP_TRY(expr)                                                                                       \
    do {                                                                                                    \
        hipError_t e_ = (expr);                                                                             \
        if (e_ != hipSuccess) return fail(KMPGPU_EHIP, "%s failed: %s", #expr, hipGetErrorString(e_));     \
    } while (0)

/* A device allocation or upload that failed: KMPGPU_ENOMEM where the memory ran out, the runtime's error state cleared.  fmt says what
 * was being taken; the runtime's own text follows it. */
int alloc_fail(hipError_t e, const char *fmt, ...)
{
    (void)hipGetLastError();
    char what[384];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(what, sizeof what, fmt, ap);
    va_end(ap);
    return fail(e == hipErrorOutOfMemory ? KMPGPU_ENOMEM : KMPGPU_EHIP, "%s: %s", what, hipGetErrorString(e));
}

/* Failure function, as kmp_prefix (serial.c:217-238). */
void failure_table(const uint8_t *pat, uint32_t m, uint8_t *out)
{
    out[0] = 0;
    uint32_t j = 0;
    for (uint32_t i = 1; i < m;) {
        if (pat[i] == pat[j]) { out[i++] = (uint8_t)++j; }
        else if (j) { j = out[j - 1]; }
        else { out[i++] = 0; }
    }
}

}  // namespace

struct kmpgpu_ctx {
    int          device = 0;
    hipStream_t  own_stream = nullptr;
    hipStream_t  stream = nullptr;
    int          cu_count = 256;

    /* patterns */
    uint32_t              n_pat = 0;
    kmp_pattern_dev      *d_patterns = nullptr;     /* [n_pat], file order; a KMPGPU_PAT_NOCASE pattern of set 1 is stored folded */
    /* fused multi-pattern pass: the eligible patterns in groups of at most KMP_MULTI_MAX_UNIQUE distinct ones, one read
     * of the arena per group */
    struct FusedGroup {
        uint32_t *d_tables = nullptr;        /* layout: kmp_device.h KMP_MULTI_*                        */
        uint32_t *d_ids = nullptr;           /* [n_ids] pattern indices counted by this group            */
        uint32_t *d_rows = nullptr;          /* [n_ids] their unique-pattern row                         */
        uint32_t *d_uid_first = nullptr, *d_uid_ids = nullptr;   /* row -> pattern indices (offset emission): CSR */
        uint32_t  words = 0, n_unique = 0, cshift = 0, bmask = 0, n_ones = 0, ones = 0, n_ids = 0;   /* cshift: a plain group's short patterns, a classed one's class shift */
        bool      classed = false;
    };
    /* The passes of one set of patterns over one arena: sets[0] holds the case-sensitive patterns (and the KMPGPU_PAT_NOCASE ones
     * without an ASCII letter, which are the same either way) and scans d_arena; sets[1] the other KMPGPU_PAT_NOCASE patterns,
     * folded, and scans the folded copy d_fold.  Both write their patterns' counts, by pattern index, into the same buffer. */
    struct PatternSet {
        uint32_t              n = 0;                 /* patterns in the set                                     */
        uint32_t             *d_ids = nullptr;       /* [n]: long patterns (m >= 4) first, then short           */
        uint32_t              n_long = 0, n_short = 0;
        std::vector<FusedGroup> fused_groups;
        uint32_t              n_multi_unique = 0;    /* distinct eligible patterns over all groups              */
        uint32_t             *d_rest_ids = nullptr;  /* [rest_long + rest_short] everything else, long first    */
        uint32_t              rest_long = 0, rest_short = 0;
    };
    PatternSet            sets[2];

    /* the folded copy of the arena for sets[1] (kmp_fold.hip): same offsets as d_arena, [0, end of the furthest slot) */
    uint8_t        *d_fold = nullptr;
    uint64_t        fold_cap = 0;
    bool            fold_stale = true;                /* d_arena has changed since the last fold */
    uint64_t        fold_end = 0;                     /* end of the furthest slot where known (host-side index); 0: ask the device */

    /* arena */
    const uint8_t  *d_arena = nullptr;
    const uint64_t *d_off = nullptr;
    const uint32_t *d_len = nullptr;
    uint64_t        arena_bytes = 0, n_pkts = 0, payload_bytes = 0;
    bool            uniform = false;                  /* every payload has the same length, slots back to back */
    bool            packed = false;                   /* slots back to back (any lengths): flat streaming with bitmap + plan */
    bool            pad_clean = false;                /* packed arena whose slot padding is all 0x00 (kmp_check_padding_kernel) */
    uint64_t        span_end = 0;                     /* end offset of the last slot */
    unsigned long long *d_bitmap = nullptr;           /* one bit per 16-byte slot: a payload starts here */
    uint4          *d_plan = nullptr;                 /* kmp_plan_entry[plan_waves + 1], 16 bytes each */
    uint64_t        plan_waves = 0, plan_cap = 0;
    uint32_t       *d_pool = nullptr;                 /* fused pass: next pool unit of every region */
    uint64_t        pool_cap = 0;
    uint4          *d_uplan = nullptr;                /* fused pass: kmp_plan_entry[uplan_units + 1], the work units of its blocks' regions */
    uint64_t        uplan_units = 0, uplan_cap = 0;
    kmp_plan_shape  uplan_shape{};                    /* what d_uplan was cut for */
    int             fused_unit = 0;                   /* KMPGPU_OPT_FUSED_UNIT */
    int             whole_payload = 0;                /* KMPGPU_OPT_WHOLE_PAYLOAD: pass state, read when a pass is enqueued */
    uint64_t        uni_off0 = 0;
    uint32_t        uni_stride = 0, uni_len = 0;
    uint8_t        *owned_arena = nullptr;
    uint64_t       *owned_off = nullptr;
    uint32_t       *owned_len = nullptr;
    uint64_t        cap_arena = 0, cap_pkts = 0;      /* capacities of the owned buffers (reused by the next load) */
    uint64_t        bitmap_cap = 0;                   /* words d_bitmap holds (kept from load to load: a streamed capture loads batch after batch) */
    bool            bitmap_live = false;              /* d_bitmap describes the arena that is attached now */
    /* scratch of kmpgpu_load_frames, kept between calls for the same reason (hipMalloc / hipFree per batch would synchronise
     * the device under the other context's scan): the frames' bytes, their offsets / captured lengths, the scan workspace, the
     * payloads' source offsets, the totals */
    uint8_t        *fr_file = nullptr, *fr_ws = nullptr;
    uint64_t       *fr_off = nullptr, *fr_src = nullptr;
    uint32_t       *fr_cl = nullptr;
    unsigned long long *fr_tot = nullptr;
    bool            fr_pending = false;               /* kmpgpu_load_frames_begin has enqueued an upload that kmpgpu_load_frames_finish has not taken yet */
    uint64_t        fr_n = 0, fr_span = 0, fr_span_lo = 0;
    int             fr_tcp = 0;
    uint64_t        fr_file_cap = 0, fr_off_cap = 0, fr_cl_cap = 0, fr_ws_cap = 0, fr_src_cap = 0;

    /* results */
    unsigned long long *d_partials = nullptr;
    uint64_t            partials_cap = 0;             /* elements */
    unsigned long long *d_counts = nullptr;
    uint32_t           *d_err = nullptr;              /* [2] validation flags */
    unsigned long long *d_sum = nullptr;              /* [6] payload bytes, offset 0, stride, length 0, end of last slot */
    uint64_t           *h_counts = nullptr;           /* pinned */
    size_t              h_counts_cap = 0;
    unsigned long long *h_small = nullptr;            /* pinned, 16 words: where the loaders read small device results back (a copy to pageable
                                                         memory goes through the runtime's blocking staging path) */
    unsigned long long *d_marks = nullptr;            /* the marking pass: hit matrix [n_pat + n_rel + n_chains + n_hdr + n_bt + n_rx + n_links][stride], then pkt_counts[n_pat], any[stride], counts[n_pat], rel_pkt_counts[n_rel], chain_pkt_counts[n_chains], hdr_pkt_counts[n_hdr], bt_pkt_counts[n_bt], rx_pkt_counts[n_rx], link_pkt_counts[n_links] */
    uint64_t            marks_cap = 0;                /* words */
    /* kmpgpu_set_rules / kmpgpu_scan_rules: the rules as the kernel reads them (kmp_launch.h, kmp_launch_rules) and the results */
    uint32_t            n_rules = 0;
    uint4              *d_rule_heads = nullptr, *d_rule_quads = nullptr;
    unsigned long long *d_rule_out = nullptr;         /* rule rows [n_rules][stride], then rule_pkt_counts[n_rules], any[stride] */
    uint64_t            rule_out_cap = 0;             /* words */
    /* kmpgpu_set_windows: {first, last} per pattern index as the emitters read it (kmp_launch.h, emit_windows); NULL: no windows set, or
     * every one of them the default -- the emitting passes then run as they do without */
    uint2              *d_windows = nullptr;
    /* kmpgpu_set_relations: {a, b, dmin, dmax} per relation as the relation kernel reads it (kmp_launch.h, kmp_launch_relations); relation
     * q is row n_pat + q of the hit matrix and term n_pat + q of a rule.  pat_fold[i]: pattern i is one of sets[1], its bytes are compared
     * in d_fold */
    uint32_t            n_rel = 0;
    uint4              *d_relations = nullptr;
    std::vector<uint8_t> pat_fold;
    /* kmpgpu_set_chains: KMPGPU_CHAIN_MAX link records per chain as the chain kernel reads them (kmp_launch.h, kmp_launch_chains); chain c
     * is row n_pat + n_rel + c of the hit matrix and term n_pat + n_rel + c of a rule */
    uint32_t            n_chains = 0;
    uint4              *d_chains = nullptr;
    /* kmpgpu_set_headers: three 16-byte records per predicate as the header kernel reads them (kmp_launch.h, kmp_launch_headers); predicate q
     * is row n_pat + n_rel + n_chains + q of the hit matrix and term n_pat + n_rel + n_chains + q of a rule */
    uint32_t            n_hdr = 0;
    uint4              *d_headers = nullptr;
    /* kmpgpu_set_bytetests: two 16-byte records per test as the byte-test kernels read them, then the indices of the n_bt_rel relative tests
     * (kmp_launch.h, kmp_launch_bytetests); bt_reach: the largest offset + nbytes of the absolute ones.  Test q is row
     * n_pat + n_rel + n_chains + n_hdr + q of the hit matrix and term n_pat + n_rel + n_chains + n_hdr + q of a rule */
    uint32_t            n_bt = 0, n_bt_rel = 0, bt_reach = 0;
    uint4              *d_bytetests = nullptr;
    /* kmpgpu_set_regexes: the expressions' tables in tiles of KMP_RX_TILE as the regex kernel reads them (kmp_regex.h, kmp_launch_regexes).
     * Expression q is row n_pat + n_rel + n_chains + n_hdr + n_bt + q of the hit matrix and that term of a rule */
    uint32_t            n_rx = 0;
    uint4              *d_regexes = nullptr;
    /* ... and of those the ones under KMPGPU_RX_GROUPS once more, in tiles of KMP_RXG_TILE for their own kernel (kmp_launch_regex_groups) */
    uint32_t            n_rx_groups = 0;
    uint4              *d_regex_groups = nullptr;
    /* kmpgpu_set_links / kmpgpu_link_rows: the link rows [n_links][links_stride] as kmpgpu_link_rows translated them, copied behind every
     * marking pass into rows n_pat + n_rel + n_chains + n_hdr + n_bt + n_rx + q of the hit matrix; link q is that term of a rule.
     * link_filled[q]: the row holds a verdict on the arena that is attached now (release_arena unfills; a filled link implies links_stride
     * is the stride of the marking pass).  rule_links: the links the rules name, ascending (kmpgpu_set_rules).  d_link_ws: the map a caller
     * gave on the host and the ranks of a bitmap (kmp_link_rank_bytes) */
    uint32_t            n_links = 0, n_links_filled = 0;
    unsigned long long *d_links = nullptr;
    uint64_t            links_cap = 0, links_stride = 0;          /* words */
    std::vector<uint8_t>  link_filled;
    std::vector<uint32_t> rule_links;
    uint8_t            *d_link_ws = nullptr;
    uint64_t            link_ws_cap = 0;
    /* the per-payload metadata the predicates are decided from (kmpgpu_pkt_meta, 16 bytes each), in payload order.  It belongs to the arena:
     * has_meta falls with it (release_arena), the buffer is kept for the next one */
    uint4              *d_meta = nullptr;
    uint64_t            meta_cap = 0;
    bool                has_meta = false;
    int                 keep_meta = 0;                /* KMPGPU_OPT_KEEP_META, read when a load of frames is begun */
    bool                fr_meta = false;              /* ... and what the load under way was begun with */
    /* kmpgpu_scan_alerts: the kept prefix of the last pass's list, 16 bytes per record (kmp_launch.h, kmp_launch_alerts_fill); alerts_valid:
     * a list exists -- an alerts pass has ended well and neither the arena nor the patterns have changed since */
    uint4              *d_alerts = nullptr;
    uint64_t            alerts_cap = 0, alerts_kept = 0;
    bool                alerts_valid = false;
    /* kmpgpu_flows_build: the hash table [flow_slots] and the lowest payload of every slot's flow [flow_slots], slot_of / flow_of [n_pkts]
     * (one array), the records [n_flows]; kmpgpu_scan_flows: the folded matrix; kmpgpu_flows_select: the payload bitmap and the uploaded
     * flow bitmap behind it.  flows_valid: flows are built, and neither the arena nor its metadata have changed since (drop_flows) */
    uint32_t           *d_flow_table = nullptr, *d_flow_first = nullptr, *d_flow_of = nullptr;
    uint64_t            flow_table_cap = 0, flow_first_cap = 0, flow_of_cap = 0;
    kmpgpu_flow        *d_flow_recs = nullptr;
    uint64_t            flow_recs_cap = 0;
    unsigned long long *d_flow_fold = nullptr, *d_flow_sel = nullptr;
    uint64_t            flow_fold_cap = 0, flow_sel_cap = 0;          /* words */
    uint64_t            n_flows = 0;
    bool                flows_valid = false;
    /* kmpgpu_load_decoded as dst: the changed bitmap [ceil(n_src / 64)] and, behind it, the four words its kernels count in */
    unsigned long long *d_dec_changed = nullptr;
    uint64_t            dec_changed_cap = 0;          /* words */
    /* kmpgpu_http_locate: one kmpgpu_http_span (two 16-byte units) per payload, the four words the kernel counts in behind them, and those
     * words on the host.  spans_valid: they describe the arena that is attached now (drop_spans) */
    uint4              *d_spans = nullptr;
    uint64_t            spans_cap = 0;                /* 16-byte units */
    uint64_t            http_stats[4] = {0, 0, 0, 0};
    bool                spans_valid = false;
    /* kmpgpu_dns_locate: one kmpgpu_dns_span per payload, the separator masks (two 16-byte units per payload as well), the four words
     * the kernel counts in, and those words on the host.  dns_valid: they describe the arena that is attached now, for the prefix flag
     * dns_prefix (dropped with the HTTP spans: drop_spans) */
    uint4              *d_dns = nullptr;
    uint64_t            dns_cap = 0;                  /* 16-byte units */
    uint64_t            dns_stats[4] = {0, 0, 0, 0};
    bool                dns_valid = false;
    uint32_t            dns_prefix = 0;
    /* kmpgpu_tls_locate: as the DNS spans, without a flag -- one kmpgpu_tls_span per payload, the ALPN separator masks, the four words */
    uint4              *d_tls = nullptr;
    uint64_t            tls_cap = 0;                  /* 16-byte units */
    uint64_t            tls_stats[4] = {0, 0, 0, 0};
    bool                tls_valid = false;
    int64_t             flow_slots = 0;               /* KMPGPU_OPT_FLOW_SLOTS */
    /* which build of the flows the context holds: kmpgpu_flows_build and drop_flows start a new generation, and id tells one context from
     * every other the process has made (a seam list names the context and the generation it was built from) */
    uint64_t            id = 0, flows_gen = 0;
    /* kmpgpu_load_seams, in dst: the kmpgpu_seam records and seam_flow [n_seams], the sort's buffers (kmp_seam_sort_bytes).  seams_valid: a
     * list exists, and the arena is the one it describes (drop_seams); seam_src / seam_gen: the flows it was built from */
    kmpgpu_seam        *d_seams = nullptr;
    uint32_t           *d_seam_flow = nullptr;
    uint8_t            *d_seam_sort = nullptr;
    uint64_t            seams_cap = 0, seam_flow_cap = 0, seam_sort_cap = 0;
    uint64_t            n_seams = 0, seam_src = 0, seam_gen = 0;
    bool                seams_valid = false;
    /* kmpgpu_load_streams, in dst: the kmpgpu_stream records [n_streams] and the kmpgpu_stream_pos entries [n_stream_map], one per payload
     * of the source.  streams_valid: they exist, and the arena is the one they describe (drop_streams) */
    kmpgpu_stream      *d_streams = nullptr;
    kmpgpu_stream_pos  *d_stream_map = nullptr;
    uint64_t            streams_cap = 0, stream_map_cap = 0;
    uint64_t            n_streams = 0, n_stream_map = 0;
    bool                streams_valid = false;
    /* kmpgpu_load_streams_ordered, in dst: the kmpgpu_stream_seg entries [n_stream_map] and the kmpgpu_stream_order records [n_streams], the
     * workspace of the second sort and its scans (kmp_stream_seq_ws_bytes) and the device copy of a host seq.  stream_order_valid: the
     * streams were built in sequence order (dropped with them) */
    kmpgpu_stream_seg   *d_stream_segs = nullptr;
    kmpgpu_stream_order *d_stream_orders = nullptr;
    uint8_t             *d_stream_seq_ws = nullptr;
    uint32_t            *d_stream_seq = nullptr;
    uint64_t            stream_segs_cap = 0, stream_orders_cap = 0, stream_seq_ws_cap = 0, stream_seq_cap = 0;
    bool                stream_order_valid = false;
    /* kmpgpu_set_flowbits: the two tables of kmp_pack_flowbits on the device and, on the host, which bits and which records of d_fb_acting
     * (two 16-byte units each) make up every level.  kmpgpu_scan_flowbits: the order of the payloads by flow (kmp_flowbits_order_bytes),
     * valid for the flows of generation fb_order_gen; the scan's workspace with before32[n_pkts] and flow_state[n_flows] behind it; the
     * before rows [n_bits][stride], the alert rows [n_rules][stride], rule_pkt_counts[n_rules], any[stride] */
    uint32_t            n_fb_bits = 0;
    std::vector<uint32_t> fb_level_mask, fb_level_first;
    uint4              *d_fb_acting = nullptr, *d_fb_tests = nullptr;
    uint8_t            *d_fb_order = nullptr, *d_fb_ws = nullptr;
    unsigned long long *d_fb_out = nullptr;
    uint64_t            fb_order_cap = 0, fb_ws_cap = 0, fb_out_cap = 0, fb_order_gen = 0;
    bool                fb_order_valid = false;
    /* kmpgpu_set_thresholds: the thresholds as given, grouped by track (kmp_pack_thresholds), and the final kernel's table on the device.
     * kmpgpu_scan_thresholds: the orders of the payloads by source and by destination address (the layout of d_fb_order), valid for the
     * metadata of generation thr_order_gen[]; the workspace (T, the aggregates, T in every sorted track's order, the prefix sum); the pass
     * rows [n_thr][stride], the alert rows [n_rules][stride], rule_pkt_counts[n_rules], any[stride]; the window counts where asked for.
     * meta_gen: which arena and metadata the context holds (drop_flows counts it up unless it is kmpgpu_flows_build that calls) */
    std::vector<kmpgpu_threshold> thr;
    std::vector<uint32_t> thr_by_track[4];
    bool                thr_windowed = false;
    uint32_t           *d_thr_table = nullptr;
    uint8_t            *d_thr_order[2] = {nullptr, nullptr}, *d_thr_ws = nullptr;
    unsigned long long *d_thr_out = nullptr;
    uint32_t           *d_thr_wc = nullptr;
    uint64_t            thr_order_cap[2] = {0, 0}, thr_ws_cap = 0, thr_out_cap = 0, thr_wc_cap = 0, thr_order_gen[2] = {0, 0}, meta_gen = 0;
    bool                thr_order_valid[2] = {false, false};
    bool                arena_seen = false;           /* some load has reached the context (release_arena); read by kmpgpu_scan_thresholds alone */
    /* the patterns as they were set, one record {length, flags, bytes} each: what kmpgpu_scan_flows_seams compares between two contexts */
    std::vector<uint8_t> pat_sig;

    /* options */
    int mode = 0, blocks_per_cu = 0 /* auto */, depth = 0 /* auto */, nontemporal = 1, kernel_sel = 0, fused = 2 /* auto */, accumulate = 0, repack = 1;

    /* timing */
    hipEvent_t  ev[4] = {nullptr, nullptr, nullptr, nullptr};
    kmpgpu_timing last{};
    std::vector<hipEvent_t> prof_ev;                  /* pairs */
    uint32_t    prof_cap = 0, prof_n = 0;
    bool        profiling = false;

    struct kmpgpu_comm *comm = nullptr;               /* the communicator this context is a rank of (kmpgpu_comm_*), if any */
};

static void comm_forget(kmpgpu_comm *k, kmpgpu_ctx *c);

namespace {

/* Uniform-stride arenas: the flat kernel from 512-byte payloads on; below that a chunk holds several packets and
 * the packed kernel's bitmap beats the flat kernel's arithmetic by 3-6 % (profiles/r01_flat_vs_packed.txt). */
bool use_flat(const kmpgpu_ctx *c)
{
    if (!c->uniform || c->mode != 0) return false;
    if (c->kernel_sel == 3) return true;
    return c->kernel_sel == 0 && (c->uni_len >= 512u || !c->packed || !c->bitmap_live);
}
/* Fused multi-pattern pass: explicit (1) or automatic (2): from 2 unique eligible patterns on -- 0.24 ms against
 * 2 x 0.23 ms as streaming passes over 1.5 GB (profiles/r02_multipattern.txt); the 1-byte patterns that ride along
 * do not count, a set of one eligible pattern plus 1-byte patterns keeps its streaming passes. */
bool use_fused(const kmpgpu_ctx *c, const kmpgpu_ctx::PatternSet &s)
{
    if (!c->packed || !c->bitmap_live || c->mode != 0 || c->kernel_sel == 1 || s.fused_groups.empty()) return false;
    return c->fused != 0 && s.n_multi_unique >= 2;
}

bool use_packed(const kmpgpu_ctx *c)
{
    return c->packed && c->bitmap_live && c->mode == 0 && (c->kernel_sel == 2 || ((c->kernel_sel == 0 || c->kernel_sel == 3) && !use_flat(c)));
}

/* Packets of a uniform stride after which a range starts on a 128-byte line again: wavefront ranges of a multiple of it share no cache
 * line with their neighbours.  (Long payloads: a shared line per range is noise, a range of several payloads is not.) */
uint64_t line_quantum(uint32_t stride)
{
    uint64_t g = stride, r = 128;
    while (r) { const uint64_t t = g % r; g = r; r = t; }                         /* gcd(stride, 128) */
    return stride >= 4096u ? 1 : 128 / g;
}

uint32_t grid_blocks(const kmpgpu_ctx *c, const kmpgpu_ctx::PatternSet &s, bool emit = false)
{
    /* In units of 4-wavefront blocks.  An explicit KMPGPU_OPT_BLOCKS_PER_CU means CUs x that many (the shape of rounds 1-2:
     * a persistent grid, 4 per CU for the flat kernel, 6 for the packed one); automatic: the flat and the packed kernel
     * take small ranges and as many blocks as that needs (below), the general kernel 8 per CU, the fused pass what
     * fits a CU (two of its 16-wavefront blocks = 8 of these units). */
    const bool streaming = use_flat(c) || use_packed(c);
    int fused_bpc = 7;
    if (use_fused(c, s)) {
        /* as many wavefronts as a CU holds of the kernel the pass will take (registers and the 160 KB of LDS), counted here in 4-wavefront blocks,
         * the unit the plan is cut in.  Only the first group carries 1-byte patterns; the plan follows it. */
        uint32_t waves = 64u;
        for (const kmpgpu_ctx::FusedGroup &g : s.fused_groups)
            waves = std::min(waves, kmp_multi_resident_waves(kmp_multi_kind(emit, c->pad_clean, s.fused_groups.front().n_ones), g.words, g.n_unique));
        /* ONE round of blocks: inside a block the wavefronts share its region out among themselves as they go (work units, enqueue_pass), so no
         * block ends long before the others and a second round has nothing to even out (with fixed ranges it had: 325 -> 317 us; with
         * units one round 303 / 146 / 154 us, two rounds 303 / 158 / 165 us on 1500-byte, Zipf and 64-byte packets, profiles/r03_fused_units_sweep2.txt) */
        fused_bpc = (int)std::max<uint32_t>(1u, waves / KMP_BLOCK_WAVES);
    }
    const int bpc = c->blocks_per_cu > 0 ? c->blocks_per_cu
                  : use_fused(c, s) ? fused_bpc : !streaming ? 8 : use_flat(c) ? 4 : 6;
    uint64_t need = (c->n_pkts + KMP_BLOCK_WAVES - 1) / KMP_BLOCK_WAVES;
    if (c->blocks_per_cu <= 0 && use_flat(c) && !use_fused(c, s) && c->uni_stride) {
        /* The flat kernel does NOT run as a persistent grid: a wavefront takes ~6 KiB (four 1500-byte packets) and the grid is
         * one block per four such ranges.  The hardware hands the blocks out in order as CUs free up, so at any moment the
         * whole chip reads one compact, moving window of the arena and nobody waits for a straggler at the end: 209-211 us per
         * 1.5 GB (0.89 of the HBM peak) against 223-234 us with four resident blocks per CU and 366 KB per wavefront
         * (profiles/r02_flat_grid.txt).  Capped so that blocks x patterns stays below 2^22 (partial counts; a launch of 2^30 threads). */
        const uint64_t q = line_quantum(c->uni_stride);                           /* ranges start on 128-byte lines */
        const uint64_t ppw = std::max<uint64_t>(6144 / c->uni_stride / q * q, q);        /* about 6 KiB, a multiple of q packets (1504-byte slots: 4) */
        uint64_t bx = (c->n_pkts + KMP_BLOCK_WAVES * ppw - 1) / (KMP_BLOCK_WAVES * ppw);
        const uint64_t max_bx = std::max<uint64_t>((1ull << 22) / std::max<uint32_t>(c->n_pat, 1u), (uint64_t)c->cu_count * 4u);
        bx = std::min(bx, max_bx);
        return (uint32_t)std::max<uint64_t>(bx, 1);
    }
    if (c->blocks_per_cu <= 0 && use_packed(c) && !use_fused(c, s)) {
        /* The packed kernel likewise: ~16 KiB per wavefront and as many blocks as that takes, handed out in order by the
         * hardware (its per-range set-up -- plan entry, bitmap words -- is heavier than the flat kernel's, 6 KiB ranges cost
         * more than they gain): Zipf 64..9000 B 109 -> 105 us per 0.67 GB, 64-byte payloads 155 -> 143 us per 0.77 GB
         * (profiles/r02_flat_grid.txt). */
        const uint64_t span = c->span_end - c->uni_off0;
        uint64_t bx = std::min<uint64_t>(need, (span + KMP_BLOCK_WAVES * 16384ull - 1) / (KMP_BLOCK_WAVES * 16384ull));
        bx = std::min<uint64_t>(bx, std::max<uint64_t>((1ull << 22) / std::max<uint32_t>(c->n_pat, 1u), (uint64_t)c->cu_count * 6u));
        return (uint32_t)std::max<uint64_t>(bx, 1);
    }
    if (streaming && c->blocks_per_cu <= 0) {
        /* small captures: give every wavefront at least 8 KiB to stream instead of launching
         * thousands of nearly empty wavefronts per pattern */
        const uint64_t span = c->span_end - c->uni_off0;
        const uint64_t per_wave = use_fused(c, s) ? 2048ull : 8192ull;      /* the fused pass does ~10x the work per byte */
        need = std::min<uint64_t>(need, (span + KMP_BLOCK_WAVES * per_wave - 1) / (KMP_BLOCK_WAVES * per_wave));
    }
    uint64_t cap = (uint64_t)c->cu_count * (uint64_t)bpc;
    uint64_t b = std::min(need, cap);
    return (uint32_t)std::max<uint64_t>(b, 1);
}

/* A device buffer of at least `want` elements, kept between calls: taken anew only when it is too small -- a batch that fits the buffer of
 * the one before costs no hipMalloc and no hipFree (either synchronises the device).  EXACT: what is asked for (a buffer whose size follows
 * from the arena or the grid); EIGHTH: an eighth more (one that follows the batches of a streamed capture, which vary a little). */
enum Headroom { EXACT, EIGHTH };

template <typename T>
hipError_t grow_buffer(T **p, uint64_t *cap, uint64_t want, Headroom headroom)
{
    if (*p && *cap >= want) return hipSuccess;
    if (*p) { const hipError_t e = hipFree(*p); *p = nullptr; *cap = 0; if (e != hipSuccess) return e; }
    const uint64_t take = headroom == EIGHTH ? want + want / 8 + 1 : want;
    const hipError_t e = hipMalloc((void **)p, (size_t)take * sizeof(T));
    if (e == hipSuccess) *cap = take;
    return e;
}

template <typename T>
void free_buffer(T **p, uint64_t *cap = nullptr)
{
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    if (cap) *cap = 0;
}

void free_pattern_set(kmpgpu_ctx::PatternSet &s)
{
    for (kmpgpu_ctx::FusedGroup &g : s.fused_groups)
        for (uint32_t *p : {g.d_tables, g.d_ids, g.d_rows, g.d_uid_first, g.d_uid_ids})
            if (p) (void)hipFree(p);
    s.fused_groups.clear();
    s.n_multi_unique = 0;
    free_buffer(&s.d_ids);
    free_buffer(&s.d_rest_ids);
    s.n = s.n_long = s.n_short = s.rest_long = s.rest_short = 0;
}

/* The set a scan reports the grid of (kmpgpu_timing.grid_blocks): the case-sensitive one, or the nocase one when it is alone. */
const kmpgpu_ctx::PatternSet &primary_set(const kmpgpu_ctx *c) { return c->sets[0].n || !c->sets[1].n ? c->sets[0] : c->sets[1]; }

/* the flow-bit ops go with the rules their indices refer to */
void drop_flowbits(kmpgpu_ctx *c)
{
    free_buffer(&c->d_fb_acting);
    free_buffer(&c->d_fb_tests);
    c->fb_level_mask.clear();
    c->fb_level_first.clear();
    c->n_fb_bits = 0;
}

/* ... and so do the thresholds */
void drop_thresholds(kmpgpu_ctx *c)
{
    free_buffer(&c->d_thr_table);
    c->thr.clear();
    for (auto &v : c->thr_by_track) v.clear();
    c->thr_windowed = false;
}

/* the rules go with the pattern set their indices refer to */
void drop_rules(kmpgpu_ctx *c)
{
    free_buffer(&c->d_rule_heads);
    free_buffer(&c->d_rule_quads);
    c->n_rules = 0;
    c->rule_links.clear();
    drop_flowbits(c);
    drop_thresholds(c);
}

/* so do the windows */
void drop_windows(kmpgpu_ctx *c) { free_buffer(&c->d_windows); }

/* ... and the relations */
void drop_relations(kmpgpu_ctx *c)
{
    free_buffer(&c->d_relations);
    c->n_rel = 0;
}

/* ... and the chains */
void drop_chains(kmpgpu_ctx *c)
{
    free_buffer(&c->d_chains);
    c->n_chains = 0;
}

/* ... and the header predicates */
void drop_headers(kmpgpu_ctx *c)
{
    free_buffer(&c->d_headers);
    c->n_hdr = 0;
}

/* ... and the byte tests */
void drop_bytetests(kmpgpu_ctx *c)
{
    free_buffer(&c->d_bytetests);
    c->n_bt = c->n_bt_rel = c->bt_reach = 0;
}

/* ... and the expressions */
void drop_regexes(kmpgpu_ctx *c)
{
    free_buffer(&c->d_regexes);
    free_buffer(&c->d_regex_groups);
    c->n_rx = c->n_rx_groups = 0;
}

/* every link is unfilled again: the arena its verdicts were about goes, or the family is set anew.  The buffer is kept for the next fill */
void unfill_links(kmpgpu_ctx *c)
{
    std::fill(c->link_filled.begin(), c->link_filled.end(), (uint8_t)0);
    c->n_links_filled = 0;
}

/* ... and the links */
void drop_links(kmpgpu_ctx *c)
{
    free_buffer(&c->d_links, &c->links_cap);
    c->link_filled.clear();
    c->n_links = c->n_links_filled = 0;
    c->links_stride = 0;
}

/* the flows go with the arena and its metadata; their buffers are kept for the next build */
void drop_flows(kmpgpu_ctx *c, bool rebuild = false)
{
    c->flows_valid = false;
    c->n_flows = 0;
    c->flows_gen++;                                /* a seam list built from them is none of the next build's */
    if (!rebuild) c->meta_gen++;                   /* the arena or its metadata change: the thresholds' address orders are none of the next one's */
}

/* the HTTP, DNS and TLS spans go with the arena whose payloads they describe; their buffers are kept for the next locate */
void drop_spans(kmpgpu_ctx *c) { c->spans_valid = c->dns_valid = c->tls_valid = false; }

/* the seam list goes with the arena it describes; its buffers are kept for the next build */
void drop_seams(kmpgpu_ctx *c)
{
    c->seams_valid = false;
    c->n_seams = 0;
}

/* the stream records and the map go with the arena they describe; their buffers are kept for the next build */
void drop_streams(kmpgpu_ctx *c)
{
    c->streams_valid = c->stream_order_valid = false;
    c->n_streams = c->n_stream_map = 0;
}

/* the patterns and all that is built on them */
void release_patterns(kmpgpu_ctx *c)
{
    free_buffer(&c->d_patterns);
    free_buffer(&c->d_counts);
    free_pattern_set(c->sets[0]);
    free_pattern_set(c->sets[1]);
    drop_rules(c);                                 /* their indices meant these patterns */
    drop_windows(c);                               /* ... and so did the windows' */
    drop_relations(c);                             /* ... and the relations' */
    drop_chains(c);                                /* ... and the chains' */
    drop_headers(c);                               /* ... and the header predicates sit behind all of them */
    drop_bytetests(c);                             /* ... and the byte tests' anchors meant these patterns */
    drop_regexes(c);                               /* ... and so did the expressions' gates */
    drop_links(c);                                 /* ... and the links sit behind all of them */
    c->pat_fold.clear();
    c->pat_sig.clear();
    c->alerts_valid = false;                       /* the list named their rows */
}

/* The context's own arena / offset / length buffers. */
void free_owned_arena(kmpgpu_ctx *c)
{
    free_buffer(&c->owned_arena, &c->cap_arena);
    free_buffer(&c->owned_off, &c->cap_pkts);
    free_buffer(&c->owned_len);
}

bool owned_arena_holds(const kmpgpu_ctx *c, uint64_t bytes, uint64_t n) { return c->owned_arena && c->cap_arena >= bytes && c->cap_pkts >= n; }

/* They hold `bytes` and `n` payloads: kept when they do already (streamed captures load batch after batch), otherwise taken anew, all three,
 * exactly or with an eighth of headroom.  On failure all three are freed: the context owns nothing and stays usable. */
hipError_t ensure_owned_arena(kmpgpu_ctx *c, uint64_t bytes, uint64_t n, Headroom headroom)
{
    if (owned_arena_holds(c, bytes, n)) return hipSuccess;
    free_owned_arena(c);
    const uint64_t take_b = bytes + (headroom == EIGHTH ? bytes / 8 : 0), take_n = n + (headroom == EIGHTH ? n / 8 : 0);
    hipError_t e = hipMalloc(&c->owned_arena, take_b);
    if (e == hipSuccess) e = hipMalloc(&c->owned_off, take_n * sizeof(uint64_t));
    if (e == hipSuccess) e = hipMalloc(&c->owned_len, take_n * sizeof(uint32_t));
    if (e != hipSuccess) { free_owned_arena(c); return e; }
    c->cap_arena = take_b; c->cap_pkts = take_n;
    return hipSuccess;
}

void release_arena(kmpgpu_ctx *c, bool keep_buffers = false)
{
    if (!keep_buffers) free_owned_arena(c);
    c->arena_seen = true;                             /* (every load comes through here first) */
    c->d_arena = nullptr; c->d_off = nullptr; c->d_len = nullptr;
    c->arena_bytes = c->n_pkts = c->payload_bytes = 0;
    c->uniform = false; c->packed = false; c->pad_clean = false; c->plan_waves = 0; c->uplan_units = 0;
    c->bitmap_live = false;                           /* the buffer itself (1/128 of an arena) is kept for the next arena */
    c->fold_stale = true; c->fold_end = 0;            /* (so is the fold buffer) */
    c->alerts_valid = false;                          /* the list of kmpgpu_scan_alerts named this arena's payloads */
    c->has_meta = false;                              /* the metadata described its payloads (the buffer is kept too) */
    drop_flows(c);                                    /* ... and the flows grouped them */
    drop_seams(c);                                    /* ... and the seam list said which of src's payloads they join */
    drop_spans(c);                                    /* ... and the HTTP spans where their fields lie */
    drop_streams(c);                                  /* ... and the stream records which of them each stream is made of */
    unfill_links(c);                                  /* ... and the links' verdicts were about them */
}

/* Host ranges pinned through kmpgpu_host_register.  One copy must not straddle two registrations (the runtime refuses it), and a
 * capture is pinned window by window: uploads are cut at the registrations' boundaries. */
std::mutex g_pinned_mu;
std::map<uintptr_t, size_t> g_pinned;

hipError_t upload_split(void *dst, const uint8_t *src, uint64_t n, hipStream_t st)
{
    std::vector<std::pair<uint64_t, uint64_t>> pieces;          /* (offset, length) */
    {
        std::lock_guard<std::mutex> lock(g_pinned_mu);
        if (g_pinned.empty()) pieces.emplace_back(0, n);
        else {
            uint64_t pos = 0;
            while (pos < n) {
                const uintptr_t a = (uintptr_t)src + pos;
                uint64_t len = n - pos;
                auto it = g_pinned.upper_bound(a);                /* first registration that starts behind a */
                if (it != g_pinned.begin()) {
                    auto in = std::prev(it);
                    if (a < in->first + in->second) len = std::min<uint64_t>(len, in->first + in->second - a);       /* inside one: up to its end */
                    else if (it != g_pinned.end()) len = std::min<uint64_t>(len, it->first - a);                     /* pageable stretch up to the next */
                } else if (it != g_pinned.end()) len = std::min<uint64_t>(len, it->first - a);
                pieces.emplace_back(pos, len);
                pos += len;
            }
        }
    }
    for (const auto &p : pieces) {
        const hipError_t e = hipMemcpyAsync((uint8_t *)dst + p.first, src + p.first, p.second, hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

void release_frame_scratch(kmpgpu_ctx *c)
{
    free_buffer(&c->fr_file, &c->fr_file_cap); free_buffer(&c->fr_ws, &c->fr_ws_cap); free_buffer(&c->fr_off, &c->fr_off_cap);
    free_buffer(&c->fr_src, &c->fr_src_cap); free_buffer(&c->fr_cl, &c->fr_cl_cap); free_buffer(&c->fr_tot);
}

/* What the passes keep from one to the next: every buffer that grow_buffer sizes for them (the frame scratch and the owned arena have
 * their own release above). */
void release_pass_buffers(kmpgpu_ctx *c)
{
    free_buffer(&c->d_bitmap, &c->bitmap_cap); free_buffer(&c->d_plan, &c->plan_cap); free_buffer(&c->d_uplan, &c->uplan_cap);
    free_buffer(&c->d_pool, &c->pool_cap); free_buffer(&c->d_partials, &c->partials_cap); free_buffer(&c->d_fold, &c->fold_cap);
    free_buffer(&c->d_marks, &c->marks_cap); free_buffer(&c->d_rule_out, &c->rule_out_cap); free_buffer(&c->d_alerts, &c->alerts_cap);
    free_buffer(&c->d_meta, &c->meta_cap); c->has_meta = false;
    free_buffer(&c->d_flow_table, &c->flow_table_cap); free_buffer(&c->d_flow_first, &c->flow_first_cap); free_buffer(&c->d_flow_of, &c->flow_of_cap);
    free_buffer(&c->d_flow_recs, &c->flow_recs_cap); free_buffer(&c->d_flow_fold, &c->flow_fold_cap); free_buffer(&c->d_flow_sel, &c->flow_sel_cap);
    free_buffer(&c->d_dec_changed, &c->dec_changed_cap); free_buffer(&c->d_link_ws, &c->link_ws_cap);
    free_buffer(&c->d_spans, &c->spans_cap); free_buffer(&c->d_dns, &c->dns_cap); free_buffer(&c->d_tls, &c->tls_cap); drop_spans(c);
    drop_flows(c);
    free_buffer(&c->d_seams, &c->seams_cap); free_buffer(&c->d_seam_flow, &c->seam_flow_cap); free_buffer(&c->d_seam_sort, &c->seam_sort_cap);
    drop_seams(c);
    free_buffer(&c->d_streams, &c->streams_cap); free_buffer(&c->d_stream_map, &c->stream_map_cap);
    free_buffer(&c->d_stream_segs, &c->stream_segs_cap); free_buffer(&c->d_stream_orders, &c->stream_orders_cap);
    free_buffer(&c->d_stream_seq_ws, &c->stream_seq_ws_cap); free_buffer(&c->d_stream_seq, &c->stream_seq_cap);
    drop_streams(c);
    free_buffer(&c->d_fb_order, &c->fb_order_cap); free_buffer(&c->d_fb_ws, &c->fb_ws_cap); free_buffer(&c->d_fb_out, &c->fb_out_cap);
    c->fb_order_valid = false;
    free_buffer(&c->d_thr_order[0], &c->thr_order_cap[0]); free_buffer(&c->d_thr_order[1], &c->thr_order_cap[1]);
    free_buffer(&c->d_thr_ws, &c->thr_ws_cap); free_buffer(&c->d_thr_out, &c->thr_out_cap); free_buffer(&c->d_thr_wc, &c->thr_wc_cap);
    c->thr_order_valid[0] = c->thr_order_valid[1] = false;
    c->alerts_valid = false;
    c->bitmap_live = false; c->plan_waves = c->uplan_units = 0; c->fold_stale = true;
}

/* The fold buffer holds at least `bytes` (an arena's size): grown where the other buffers are, only while a pattern needs it. */
int grow_fold(kmpgpu_ctx *c, uint64_t bytes)
{
    if (!c->sets[1].n || !bytes) return KMPGPU_OK;
    const uint64_t want = (bytes + 15u) & ~15ull;
    const hipError_t e = grow_buffer(&c->d_fold, &c->fold_cap, want, EIGHTH);
    if (e != hipSuccess) return alloc_fail(e, "the fold buffer of the nocase patterns (%llu bytes) could not be allocated", (unsigned long long)bytes);
    return KMPGPU_OK;
}

/* Before a pass of the nocase set: d_fold = fold(d_arena) over [0, end of the furthest slot), once per arena (enqueued on the
 * context's stream; neither a launch of kmpgpu_timing nor one kmpgpu_profile_* records). */
int ensure_fold(kmpgpu_ctx *c)
{
    if (!c->fold_stale) return KMPGPU_OK;
    uint64_t end = c->packed ? c->span_end : c->fold_end;          /* slots back to back: the last one is the furthest */
    if (!end) {
        /* an index that is not in arena order (an arena scanned in place): its furthest slot, asked once */
        HIP_TRY(hipMemsetAsync(c->d_sum + 5, 0, sizeof(unsigned long long), c->stream));
        HIP_TRY(kmp_launch_slot_end(c->d_off, c->d_len, c->n_pkts, c->d_sum + 5, c->stream));
        HIP_TRY(hipMemcpyAsync(c->h_small + 15, c->d_sum + 5, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        end = c->fold_end = c->h_small[15];
    }
    if (end > c->arena_bytes) return fail(KMPGPU_EINVAL, "kmpgpu_scan: a slot ends behind the arena");
    if (c->fold_cap < end) {
        int rc = grow_fold(c, end);
        if (rc) return rc;
    }
    HIP_TRY(kmp_launch_fold(c->d_arena, c->d_fold, end, c->stream));
    c->fold_stale = false;
    return KMPGPU_OK;
}

/* What a loader has found out about an index it has checked against the layout contract: by kmpgpu_load_arena's loop over a host index,
 * or by kmp_validate_index_kernel over one that lies on the device (validate_index). */
struct IndexFacts {
    uint64_t payload_bytes = 0;
    bool     uniform = false;                         /* every payload has the same length, slots at one stride */
    uint64_t off0 = 0;                                /* the first payload's offset, the stride and the length of a uniform index */
    uint32_t stride = 0, len0 = 0;
    bool     packed = false;                          /* slots back to back */
    uint64_t span_end = 0;                            /* end of the last slot */
    uint64_t fold_end = 0;                            /* end of the furthest slot (the last one only when the index is in arena order); 0: not known */
};

int install_arena(kmpgpu_ctx *c, const uint8_t *arena, const uint64_t *off, const uint32_t *len, uint64_t arena_bytes, uint64_t n_pkts,
                  const IndexFacts &f, bool wrote_padding);

/* An arena whose slots are not back to back (gaps, shuffled order) is copied once into a packed one owned by the context, so that
 * the streaming kernels apply to it too: by prepare_packed under KMPGPU_OPT_REPACK (default on), and whatever that option says by
 * the passes that run on the streaming kernels only. */
int repack_arena(kmpgpu_ctx *c)
{
    uint8_t *ws = nullptr, *na = nullptr;
    uint64_t *noff = nullptr;
    uint32_t *nlen = nullptr;
    unsigned long long *d_tot = nullptr, tot[2] = {0, 0};
    auto drop = [&]() { if (ws) (void)hipFree(ws); if (d_tot) (void)hipFree(d_tot); };
#define KMP_TRY3(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { drop(); if (na) (void)hipFree(na); if (noff) (void)hipFree(noff); if (nlen) (void)hipFree(nlen); \
        return fail(KMPGPU_EHIP, "%s failed: %s", #expr, hipGetErrorString(e_)); } } while (0)
    KMP_TRY3(hipMalloc(&ws, kmp_extract_ws_bytes(c->n_pkts)));
    KMP_TRY3(hipMalloc(&d_tot, 2 * sizeof(unsigned long long)));
    KMP_TRY3(kmp_launch_repack_phase1(c->d_len, c->n_pkts, ws, d_tot, c->stream));
    KMP_TRY3(hipMemcpyAsync(tot, d_tot, sizeof tot, hipMemcpyDeviceToHost, c->stream));
    KMP_TRY3(hipStreamSynchronize(c->stream));
    const uint64_t nbytes = tot[0] + 64;
    KMP_TRY3(hipMalloc(&na, nbytes));
    KMP_TRY3(hipMalloc(&noff, c->n_pkts * sizeof(uint64_t)));
    KMP_TRY3(hipMalloc(&nlen, c->n_pkts * sizeof(uint32_t)));
    KMP_TRY3(hipMemsetAsync(na + tot[0], 0, 64, c->stream));
    KMP_TRY3(hipMemcpyAsync(nlen, c->d_len, c->n_pkts * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
    KMP_TRY3(kmp_launch_repack_phase2(c->d_arena, c->d_off, c->d_len, c->n_pkts, ws, na, noff, c->stream));
    KMP_TRY3(hipStreamSynchronize(c->stream));
#undef KMP_TRY3
    drop();
    /* the context now owns the packed copy; a borrowed or uploaded original is released */
    free_owned_arena(c);
    c->owned_arena = na; c->owned_off = noff; c->owned_len = nlen;
    c->cap_arena = nbytes; c->cap_pkts = c->n_pkts;
    IndexFacts f;
    f.payload_bytes = c->payload_bytes;
    f.packed = true;
    f.span_end = f.fold_end = tot[0];
    return install_arena(c, na, noff, nlen, nbytes, c->n_pkts, f, /* wrote_padding = */ false);
}

/* Side tables of the packed streaming kernel: start bitmap now, wavefront plan on first use.  wrote_padding: the loader wrote the
 * slot padding of the context's own arena itself, no check pass. */
int prepare_packed(kmpgpu_ctx *c, bool wrote_padding)
{
    if (c->n_pkts == 0) return KMPGPU_OK;
    if (!c->packed) return c->repack ? repack_arena(c) : KMPGPU_OK;          /* (which installs its packed copy and so comes back here) */
    const uint64_t words = c->arena_bytes / KMP_CHUNK + 32;              /* the group prefetch reads up to 2 * DEPTH + 1 words past the end */
    HIP_TRY(grow_buffer(&c->d_bitmap, &c->bitmap_cap, words, EXACT));
    HIP_TRY(hipMemsetAsync(c->d_bitmap, 0, words * sizeof(unsigned long long), c->stream));
    HIP_TRY(kmp_launch_build_bitmap(c->d_off, c->n_pkts, c->d_bitmap, c->stream));
    c->bitmap_live = true;
    /* slot padding: checked once; cleared when the arena is the context's own copy, otherwise the packed
     * kernel keeps fetching offset and length of a candidate's payload from the index */
    const bool own = c->owned_arena && c->d_arena == c->owned_arena;
    if (own && wrote_padding) { c->pad_clean = true; return KMPGPU_OK; }
    uint32_t dirty = 0;
    HIP_TRY(hipMemsetAsync(c->d_err, 0, sizeof(uint32_t), c->stream));
    HIP_TRY(kmp_launch_check_padding(const_cast<uint8_t *>(c->d_arena), c->d_off, c->d_len, c->n_pkts, own ? 1 : 0, c->d_err, c->stream));
    HIP_TRY(hipMemcpyAsync(c->h_small, c->d_err, sizeof dirty, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    memcpy(&dirty, c->h_small, sizeof dirty);
    c->pad_clean = own || dirty == 0;
    return KMPGPU_OK;
}

/* The one place an arena becomes the context's: the pointers (its own buffers or borrowed ones), what is known about the index, the fold
 * buffer, and the packed kernels' side tables. */
int install_arena(kmpgpu_ctx *c, const uint8_t *arena, const uint64_t *off, const uint32_t *len, uint64_t arena_bytes, uint64_t n_pkts,
                  const IndexFacts &f, bool wrote_padding)
{
    c->d_arena = arena; c->d_off = off; c->d_len = len;
    c->arena_bytes = arena_bytes; c->n_pkts = n_pkts; c->payload_bytes = f.payload_bytes;
    c->uniform = f.uniform; c->uni_off0 = f.off0; c->uni_stride = f.stride; c->uni_len = f.len0;
    c->packed = f.packed;
    c->span_end = f.span_end;
    c->fold_stale = true; c->fold_end = f.fold_end;
    c->alerts_valid = false;
    (void)grow_fold(c, arena_bytes);                  /* (a failure is reported by the first scan that needs the fold) */
    return prepare_packed(c, wrote_padding);
}

/* The layout contract, uniform / packed detection and the payload sum of an index that lies on the device (kmp_validate_index_kernel),
 * read back through the pinned words (a copy to pageable memory goes through the runtime's blocking staging path). */
int validate_index(kmpgpu_ctx *c, const char *who, const uint64_t *d_off, const uint32_t *d_len, uint64_t n_pkts, uint64_t arena_bytes, IndexFacts *f)
{
    HIP_TRY(hipMemsetAsync(c->d_err, 0, 2 * sizeof(uint32_t), c->stream));
    HIP_TRY(hipMemsetAsync(c->d_sum, 0, 6 * sizeof(unsigned long long), c->stream));
    HIP_TRY(kmp_launch_validate(d_off, d_len, n_pkts, arena_bytes, c->d_err, c->d_sum, c->stream));
    HIP_TRY(hipMemcpyAsync(c->h_small, c->d_sum, 6 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(c->h_small + 8, c->d_err, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const unsigned long long *info = c->h_small;
    uint32_t err[2];
    memcpy(err, c->h_small + 8, sizeof err);
    if (err[0] & 1u) return fail(KMPGPU_EINVAL, "%s: a payload offset is not 16-byte aligned", who);
    if (err[0] & 2u) return fail(KMPGPU_EINVAL, "%s: a payload (padded to 16 B) exceeds the arena", who);
    if (err[0] & 4u) return fail(KMPGPU_EINVAL, "%s: a payload length is above 2^30", who);
    *f = IndexFacts{};
    f->payload_bytes = info[0];
    f->uniform = ((err[1] & 1u) == 0) && info[2] >= 16 && info[2] < (1ull << 31);
    f->off0 = info[1]; f->stride = (uint32_t)info[2]; f->len0 = (uint32_t)info[3];
    f->packed = (err[1] & 2u) == 0;
    f->span_end = info[4];
    return KMPGPU_OK;
}

/* A launch that kmpgpu_profile_begin .. _end times: the next event pair, its first event recorded in front of the launch and its second
 * one (*e1; NULL while no profile runs or it is full) behind it. */
hipError_t profile_launch(kmpgpu_ctx *c, hipEvent_t *e1)
{
    *e1 = nullptr;
    if (!c->profiling || c->prof_n >= c->prof_cap) return hipSuccess;
    *e1 = c->prof_ev[2 * c->prof_n + 1];
    return hipEventRecord(c->prof_ev[2 * c->prof_n], c->stream);
}
hipError_t profile_launched(kmpgpu_ctx *c, hipEvent_t e1)
{
    if (!e1) return hipSuccess;
    c->prof_n++;
    return hipEventRecord(e1, c->stream);
}
/* ... and the two around one launch: profiled(c, [&] { return kmp_launch_...(...); }) */
template <class Launch> hipError_t profiled(kmpgpu_ctx *c, Launch launch)
{
    hipEvent_t e1;
    hipError_t e = profile_launch(c, &e1);
    if (e == hipSuccess) e = launch();
    return e == hipSuccess ? profile_launched(c, e1) : e;
}

/* Records [first, first + n) of a list of `total` on the device, `size` bytes each, to the host: what every _read call does behind its NULL
 * check.  missing: what the call says while the list is not valid; what / have: "elements" or "records", "there are" or "kept". */
int read_range(kmpgpu_ctx *c, const char *who, bool valid, const char *missing, void *out, const void *d_list, size_t size, uint64_t first,
               uint64_t n, uint64_t total, const char *what = "elements", const char *have = "there are")
{
    if (!valid) return fail(KMPGPU_ESTATE, "%s: %s", who, missing);
    if (first > total || n > total - first)
        return fail(KMPGPU_EINVAL, "%s: %s [%llu, +%llu) leave the %llu %s", who, what, (unsigned long long)first, (unsigned long long)n,
                    (unsigned long long)total, have);
    if (n == 0) return KMPGPU_OK;
    if (!out) return fail(KMPGPU_EINVAL, "%s: out is NULL", who);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(out, (const uint8_t *)d_list + first * size, (size_t)n * size, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return KMPGPU_OK;
}

/* ------------------------------------------------------------------------------------------------------------------------------------
 * The derived-arena loaders (kmpgpu_load_selected, _decoded, _base64, _fields, _dns, _tls, _seams, _streams, _streams_ordered): dst's
 * arena built out of src's on dst's stream.  Every one of them is these steps in this order, with its own launches between them
 * (DESIGN.md §3.31.1):
 *   pair_refused, the checks of its own arguments, pair_state_refused, the checks of src's state
 *   derived_begin; with a src without payloads: release_arena and out
 *   its scratch; ev[2]; its launches, each through profiled(); read_totals
 *   release_arena (seams and streams: right behind derived_begin); with nothing to hold: derived_finish(record) and out
 *   take_arena; its buffers; its index and write launches; ev[3]; install_owned; derived_finish; its state
 * ------------------------------------------------------------------------------------------------------------------------------------ */

/* The refusals in front of a call's checks of its own arguments ... */
int pair_refused(const kmpgpu_ctx *dst, const kmpgpu_ctx *src, const char *who)
{
    if (!dst || !src) return fail(KMPGPU_EINVAL, "%s: ctx is NULL", who);
    if (dst == src) return fail(KMPGPU_EINVAL, "%s: dst and src are the same context (a context holds one arena)", who);
    return KMPGPU_OK;
}
/* ... and the ones behind them, in front of its checks of src's state.  what: what the call makes, for the message */
int pair_state_refused(const kmpgpu_ctx *dst, const kmpgpu_ctx *src, const char *who, const char *what)
{
    if (dst->device != src->device)
        return fail(KMPGPU_EINVAL, "%s: the contexts sit on devices %d and %d (no %s across devices)", who, dst->device, src->device, what);
    if (dst->fr_pending || src->fr_pending)
        return fail(KMPGPU_ESTATE, "%s: %s sits between kmpgpu_load_frames_begin and _finish", who, dst->fr_pending ? "dst" : "src");
    return KMPGPU_OK;
}

int derived_begin(kmpgpu_ctx *dst, kmpgpu_ctx *src)
{
    HIP_TRY(hipSetDevice(dst->device));
    HIP_TRY(hipStreamSynchronize(dst->stream));           /* the passes over the arena that is about to be replaced */
    HIP_TRY(hipStreamSynchronize(src->stream));           /* whatever src's stream still does with its arena */
    dst->last = kmpgpu_timing{};
    return KMPGPU_OK;
}

/* What the scan left in fr_tot -- tot[0] the packed bytes, tot[1] the payloads -- through the pinned words (no staging), and with
 * bitmap_words the changed / present bitmap in d_dec_changed: its four totals behind it to tot[2..6) and its words to bitmap_out (host,
 * may be NULL).  One synchronisation of the stream. */
int read_totals(kmpgpu_ctx *c, unsigned long long *tot, uint64_t bitmap_words = 0, void *bitmap_out = nullptr)
{
    HIP_TRY(hipMemcpyAsync(c->h_small, c->fr_tot, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    if (bitmap_words)
        HIP_TRY(hipMemcpyAsync(c->h_small + 2, c->d_dec_changed + bitmap_words, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    if (bitmap_words && bitmap_out)
        HIP_TRY(hipMemcpyAsync(bitmap_out, c->d_dec_changed, bitmap_words * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    memcpy(tot, c->h_small, (bitmap_words ? 6 : 2) * sizeof *tot);
    return KMPGPU_OK;
}

/* dst's own buffers for n slots that end at packed_bytes, and the 64 bytes of 0x00 behind them.  On failure dst is empty and usable. */
int take_arena(kmpgpu_ctx *c, const char *who, uint64_t packed_bytes, uint64_t n, const char *what)
{
    const uint64_t arena_bytes = packed_bytes + 64;
    const hipError_t e = ensure_owned_arena(c, arena_bytes, n, EIGHTH);
    if (e != hipSuccess)
        return alloc_fail(e, "%s: an arena of %llu bytes / %llu %s could not be allocated", who, (unsigned long long)(arena_bytes + arena_bytes / 8),
                          (unsigned long long)(n + n / 8), what);
    HIP_TRY(hipMemsetAsync(c->owned_arena + packed_bytes, 0, 64, c->stream));
    return KMPGPU_OK;
}

/* The arena a loader has written into dst's own buffers becomes dst's; one that fails the check leaves dst empty.  Every write kernel of
 * these loaders writes its slots whole: payload, then 0x00 up to the slot's end. */
int install_owned(kmpgpu_ctx *c, const char *who, uint64_t packed_bytes, uint64_t n)
{
    IndexFacts f;
    int rc = validate_index(c, who, c->owned_off, c->owned_len, n, packed_bytes + 64, &f);
    if (!rc) rc = install_arena(c, c->owned_arena, c->owned_off, c->owned_len, packed_bytes + 64, n, f, /* wrote_padding = */ true);
    if (rc) release_arena(c, true);
    return rc;
}

/* kernel_ms from ev[2] to ev[3], and the launches between them.  record: ev[3] is not on the stream yet (a result without payloads: it is
 * recorded and waited for here); otherwise the caller recorded it behind its last launch, and install_owned has waited for the stream. */
int derived_finish(kmpgpu_ctx *c, uint32_t launches, bool record)
{
    if (record) {
        HIP_TRY(hipEventRecord(c->ev[3], c->stream));
        HIP_TRY(hipEventSynchronize(c->ev[3]));
    }
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev[2], c->ev[3]));
    c->last.kernel_ms = ms; c->last.launches = launches;
    return KMPGPU_OK;
}

/* The front seams and streams share, in two halves.  Its scratch: the sort sized, fr_ws of ws_bytes, fr_tot and the sort's buffer grown;
 * nothing goes onto the stream, so a caller takes whatever else it needs and uploads only after that ... */
int flow_sort_scratch(kmpgpu_ctx *c, const kmpgpu_ctx *src, const char *who, uint64_t ws_bytes)
{
    const uint64_t n = src->n_pkts, sort_bytes = kmp_seam_sort_bytes(n, src->n_flows);
    if (!sort_bytes) return fail(KMPGPU_EHIP, "%s: the sort of %llu payloads could not be sized", who, (unsigned long long)n);
    hipError_t e = grow_buffer(&c->fr_ws, &c->fr_ws_cap, ws_bytes, EIGHTH);
    if (e == hipSuccess && !c->fr_tot) e = hipMalloc(&c->fr_tot, 2 * sizeof(unsigned long long));
    if (e == hipSuccess) e = grow_buffer(&c->d_seam_sort, &c->seam_sort_cap, sort_bytes, EIGHTH);
    if (e != hipSuccess) return alloc_fail(e, "%s: the sort's buffers (%llu bytes) could not be allocated", who, (unsigned long long)sort_bytes);
    return KMPGPU_OK;
}
/* ... and the work: ev[2], and src's payloads sorted by flow and direction in d_seam_sort. */
int sort_by_flow(kmpgpu_ctx *c, const kmpgpu_ctx *src)
{
    const uint64_t n = src->n_pkts;
    HIP_TRY(hipEventRecord(c->ev[2], c->stream));
    HIP_TRY(profiled(c, [&] { return kmp_launch_seam_keys(src->d_meta, src->d_flow_of, src->d_flow_recs, n, c->d_seam_sort, c->stream); }));
    HIP_TRY(profiled(c, [&] { return kmp_launch_seam_sort(n, src->n_flows, c->d_seam_sort, (size_t)c->seam_sort_cap, c->stream); }));
    return KMPGPU_OK;
}

/* Enqueue one full pass: scan launches (patterns grouped by "shorter than 4 bytes") + reduce. */
struct EmitTarget {
    void *out = nullptr; unsigned long long *counter = nullptr; unsigned long long cap = 0;
    unsigned long long *marks = nullptr; uint32_t mark_stride = 0;       /* kmpgpu_scan_packets: the hit matrix instead of records */
};

/* Partial counts of one set's pass: a row per pattern -- or, where the fused pass runs, a row per id of its largest group (a classed group
 * numbers its patterns by bucket class, up to 1024 ids however few patterns it has) and one per pattern that keeps a pass of its own. */
size_t part_rows(const kmpgpu_ctx *c, const kmpgpu_ctx::PatternSet &s)
{
    size_t rows = c->n_pat;
    if (use_fused(c, s)) {
        size_t max_u = 0;
        for (const kmpgpu_ctx::FusedGroup &g : s.fused_groups) max_u = std::max<size_t>(max_u, g.n_unique);
        rows = std::max<size_t>(rows, max_u + s.rest_long + s.rest_short);
    }
    return rows;
}

/* The work units of the fused pass over `span` bytes on a grid of bx 4-wavefront blocks, run as blocks of `bwaves` wavefronts. */
struct FusedPlan {
    kmp_plan_shape shape;              /* region, step, units per region, big units, pool unit: what kmp_plan_kernel cuts */
    uint64_t fblocks = 0;              /* blocks of the launch; fblocks / sides regions */
    uint32_t sides = 1;                /* blocks that share a region */
    uint64_t n_units = 0;              /* regions x shape.units */
};

/* The fused pass: one region of the arena per PAIR of blocks, in work units their wavefronts take one after the other
 * (kmp_scan_multi.hip).  Every wavefront starts with one large unit of its own, and the second half of the region
 * lies in a pool of 32 KiB units for whoever is done first (profiles/r03_fused_units_sweep4_pair_pools.txt): the SIMDs serve their wavefronts in order of age, so the
 * first wavefront of a block is through its share when the last one has a third to go, and the block that came to a CU first
 * is done when the second one has a third to go.  (Small units throughout cost more than they balance: a unit begins
 * with the dependent chain counter - entry - first loads, which the other wavefronts of the SIMD do not cover --
 * profiles/r03_tried_all_units_dynamic.txt.)
 * false: the plan does not fit 32 bits (positions inside a region and unit numbers are 32-bit, kmp_scan_multi.hip); the set then keeps its
 * streaming passes. */
bool plan_fused(uint64_t span, uint32_t bx, uint32_t bwaves, int fused_unit, FusedPlan *p)
{
    uint64_t fblocks = ((uint64_t)bx * KMP_BLOCK_WAVES + bwaves - 1u) / bwaves;
    const uint32_t sides = fblocks >= 2 ? 2u : 1u;
    fblocks -= fblocks % sides;
    const uint64_t regions = fblocks / sides;
    kmp_plan_shape sh{};
    sh.region = (((span + regions - 1) / regions) + 1023ull) & ~1023ull;
    uint64_t small = fused_unit ? (uint64_t)fused_unit : 32768ull, pool_num = 1, pool_div = 2, big = 0;
#ifdef KMP_MULTI_TUNING
    if (const char *e = getenv("KMP_FUSED_UNIT")) big = strtoull(e, nullptr, 0) & ~1023ull;          /* 0: from the pool's share */
    if (const char *e = getenv("KMP_FUSED_SMALL")) small = std::max<uint64_t>(1024ull, strtoull(e, nullptr, 0) & ~1023ull);
    if (const char *e = getenv("KMP_FUSED_TAIL_DIV")) { pool_num = 1; pool_div = std::max<uint64_t>(1ull, strtoull(e, nullptr, 0)); }
    if (const char *e = getenv("KMP_FUSED_TAIL_NUM")) pool_num = std::min<uint64_t>(pool_div, strtoull(e, nullptr, 0));
#endif
    uint64_t big_units = (uint64_t)sides * bwaves;
    /* (a small region -- a capture of a few hundred KB per block -- goes to the wavefronts whole: a unit of the pool costs a round trip
     * to the counter in global memory, which a pass of 10 us does not have) */
    const bool no_pool = sh.region < (1ull << 20) && !big;
    const uint64_t own_bytes = no_pool ? sh.region : sh.region - sh.region / pool_div * pool_num;
    sh.step = big ? big : std::max<uint64_t>(1024ull, no_pool ? ((own_bytes + big_units - 1) / big_units + 1023ull) & ~1023ull : (own_bytes / big_units) & ~1023ull);
    if (!no_pool && big_units * sh.step > sh.region) big_units = sh.region / sh.step;
    uint64_t rest = no_pool ? 0ull : sh.region - big_units * sh.step;         /* (without a pool the shares reach the region's end: kmp_plan_kernel cuts them there) */
    /* (a small region: at least two units of the pool per wavefront, or the last unit is all that is left to do for a long time) */
    if (!fused_unit) small = std::min<uint64_t>(small, std::max<uint64_t>(1024ull, (rest / (2ull * big_units ? 2ull * big_units : 1ull)) & ~1023ull));
    /* a block holds the entries of its units in LDS, KMP_MULTI_MAX_UNITS of them: a large region has larger pool units */
    const uint64_t room = KMP_MULTI_MAX_UNITS - 1u - big_units;                  /* (one entry stays free: "no such unit") */
    if ((rest + small - 1) / small > room) small = (((rest + room - 1) / room) + 1023ull) & ~1023ull;
    sh.small = (uint32_t)small;
    const uint64_t upb = big_units + (rest + small - 1) / small;
    const uint64_t n_units = regions * upb;
    if (!(sh.region < 0x7FE00000ull && n_units < (1ull << 31))) return false;
    sh.big_units = (uint32_t)big_units; sh.units = (uint32_t)upb;
    p->shape = sh; p->fblocks = fblocks; p->sides = sides; p->n_units = n_units;
    return true;
}

/* The launches of one set over `arena` (d_arena, or the folded copy for the nocase set): scan launches (patterns grouped by "shorter
 * than 4 bytes") + reduce, into d_out by pattern index. */
int enqueue_set(kmpgpu_ctx *c, const kmpgpu_ctx::PatternSet &s, const uint8_t *arena, uint32_t bx, uint32_t &nl, unsigned long long *d_out,
                bool accumulate, const EmitTarget *emit)
{
    kmp_scan_args a{};
    a.arena = arena; a.pkt_off = c->d_off; a.pkt_len = c->d_len; a.n_pkts = c->n_pkts;
    a.patterns = c->d_patterns; a.blocks_x = bx; a.depth = c->depth; /* 0: the launcher's own default */ a.mode = c->mode;
    a.nontemporal = c->nontemporal != 0;
    a.whole = c->whole_payload != 0;
    a.pad_clean = c->pad_clean;
    if (emit) {
        a.emit_out = emit->out; a.emit_counter = emit->counter; a.emit_cap = emit->cap;
        a.emit_marks = emit->marks; a.mark_stride = emit->mark_stride; a.mark_rows = c->n_pat;
        a.emit_windows = c->d_windows;               /* every launch of the pass: streaming, fused, 1-byte reads, the nocase set */
    }
    /* uniform-stride arenas take the flat streaming kernel (contiguous packet run per wavefront) */
    const uint64_t nwaves = (uint64_t)bx * KMP_BLOCK_WAVES;
    uint64_t ppw = (c->n_pkts + nwaves - 1) / nwaves;
    if (c->uniform && c->uni_stride) {
        /* start every wavefront's range on a 128-byte line so that neighbouring ranges share no cache line */
        const uint64_t q = line_quantum(c->uni_stride);
        ppw = (ppw + q - 1) / q * q;
    }
    const bool flat = use_flat(c) && ppw * c->uni_stride < (1ull << 31);
    if (flat) {
        a.arena = arena + c->uni_off0;
        a.uniform_stride = c->uni_stride; a.uniform_len = c->uni_len; a.pkts_per_wave = (uint32_t)ppw;
    }
    /* packed arenas: byte-balanced wavefront ranges (plan) + packet-start bitmap, used by the packed
     * streaming kernel (mixed lengths) and by the fused multi-pattern pass */
    const bool fused = use_fused(c, s);
    bool packed = !flat && use_packed(c);
    bool do_fused = false;
    if (fused) {
        /* its work units (plan_fused), cut at packet starts once per shape (kmp_plan_kernel), and a pool counter per region */
        const uint32_t bwaves =kmp_multi_block_waves(kmp_multi_kind(emit != nullptr, c->pad_clean, s.fused_groups.front().n_ones));
        FusedPlan fp;
        if (plan_fused(c->span_end - c->uni_off0, bx, bwaves, c->fused_unit, &fp)) {
            const kmp_plan_shape &sh = fp.shape, &o = c->uplan_shape;
            if (c->uplan_units != fp.n_units || o.step != sh.step || o.region != sh.region || o.units != sh.units || o.big_units != sh.big_units || o.small != sh.small) {
                HIP_TRY(grow_buffer(&c->d_uplan, &c->uplan_cap, fp.n_units + 1, EXACT));
                HIP_TRY(kmp_launch_plan(c->d_off, c->d_len, c->n_pkts, fp.n_units, sh, c->d_uplan, c->stream));
                c->uplan_units = fp.n_units; c->uplan_shape = sh;
            }
            HIP_TRY(grow_buffer(&c->d_pool, &c->pool_cap, fp.fblocks / fp.sides, EXACT));       /* a counter per region */
            a.fused_blocks = (uint32_t)fp.fblocks; a.units_per_block = sh.units; a.n_units = (uint32_t)fp.n_units; a.span_end = c->span_end;
            a.fused_sides = fp.sides; a.fused_pool = c->d_pool;
            a.bitmap = c->d_bitmap;
            do_fused = true;
        }
    }
    if (packed) {
        const uint64_t span = c->span_end - c->uni_off0;
        uint64_t bpw = (((span + nwaves - 1) / nwaves) + 15ull) & ~15ull;
        /* whole chunks per range where the ranges are several chunks long: equal-length small payloads then start every range on a
         * 1 KiB boundary (12 M x 64 B: 16 320-byte ranges 154-160 us, 16 384-byte ranges 142-144 us) */
        if (bpw >= 8192ull) bpw = (bpw + 1023ull) & ~1023ull;
        if (bpw >= (1ull << 30)) packed = false;
        else {
            if (c->plan_waves != nwaves) {
                HIP_TRY(grow_buffer(&c->d_plan, &c->plan_cap, nwaves + 1, EXACT));
                kmp_plan_shape sh{};
                sh.step = bpw ? bpw : 16;
                HIP_TRY(kmp_launch_plan(c->d_off, c->d_len, c->n_pkts, nwaves, sh, c->d_plan, c->stream));
                c->plan_waves = nwaves;
            }
            a.bitmap = c->d_bitmap; a.plan = c->d_plan;
        }
    }

    const uint32_t *ids = s.d_ids;
    uint32_t n_long = s.n_long, n_short = s.n_short;
    size_t part_base = 0;                         /* partial rows already used */
    if (do_fused) {
        /* one read of the arena for every group of unique patterns of 2..99 bytes (up to 256, classed groups up to 1024) */
        uint32_t max_u = 0;
        for (const kmpgpu_ctx::FusedGroup &g : s.fused_groups) {
            kmp_scan_args f = a;
            f.arena = arena;
            f.plan = c->d_uplan;
            f.fused_classed = g.classed;
            f.partials = c->d_partials;
            /* the regions' pool counters start from 0; regions without a pool (every unit is some wavefront's own) get no counter at all --
             * one that is never reset would come round after 2^32 takes, and a streamed capture is a pass per batch */
            f.fused_pool = nullptr;
            if (a.units_per_block > a.fused_sides * kmp_multi_block_waves(kmp_multi_kind(emit != nullptr, c->pad_clean, g.n_ones))) {
                HIP_TRY(hipMemsetAsync(c->d_pool, 0, (size_t)(a.fused_blocks / a.fused_sides) * sizeof(uint32_t), c->stream));
                f.fused_pool = c->d_pool;
            }
            HIP_TRY(profiled(c, [&] {
                return kmp_launch_scan_multi(f, g.d_tables, g.words, g.n_unique, g.cshift, g.bmask, g.n_ones, g.ones, g.d_uid_first, g.d_uid_ids, c->stream);
            }));
            HIP_TRY(kmp_launch_reduce(c->d_partials, bx, g.d_ids, g.n_ids, d_out, c->stream, g.d_rows, accumulate));
            ++nl;
            max_u = std::max(max_u, g.n_unique);
        }
        part_base = max_u;
        ids = s.d_rest_ids; n_long = s.rest_long; n_short = s.rest_short;
    }

    struct Group { uint32_t first, n; bool masked; } groups[2] = {{0, n_long, false}, {n_long, n_short, true}};
    for (const Group &g : groups) {
        /* gridDim.y is limited to 65535 */
        for (uint32_t done = 0; done < g.n; done += 65535u) {
            const uint32_t n = std::min(65535u, g.n - done);
            a.pat_ids = ids + g.first + done;
            a.n_ids = n;
            a.partials = c->d_partials + (part_base + g.first + done) * bx;
            a.masked = g.masked;
            /* tens of thousands of partials per pattern are added up by several blocks, which add to the counter: it starts from 0 */
            const bool sliced = (flat || packed) && kmp_reduce_is_sliced(bx);
            a.zero_counts = (sliced && !accumulate) ? d_out : nullptr;
            hipEvent_t e1;
            HIP_TRY(profile_launch(c, &e1));
            if (emit && !flat && !packed)
                return fail(KMPGPU_EINVAL, "%s: the arena could not be brought into the streaming kernels' layout",
                            emit->marks ? "kmpgpu_scan_packets" : "kmpgpu_scan_offsets");
            HIP_TRY(flat ? kmp_launch_scan_flat(a, c->stream) : packed ? kmp_launch_scan_packed(a, c->stream) : kmp_launch_scan(a, c->stream));
            HIP_TRY(profile_launched(c, e1));
            HIP_TRY(kmp_launch_reduce(a.partials, bx, a.pat_ids, n, d_out, c->stream, nullptr, accumulate, sliced));
            ++nl;
        }
    }
    return KMPGPU_OK;
}

/* Enqueue one full pass: the case-sensitive set over the arena, then the nocase set over its folded copy.  accumulate: the counts are
 * added to d_out (KMPGPU_OPT_ACCUMULATE for the counting passes; a pass that emits writes to a buffer of its own and never accumulates). */
int enqueue_pass(kmpgpu_ctx *c, uint32_t *launches, unsigned long long *d_out, bool accumulate, const EmitTarget *emit = nullptr)
{
    if (!d_out) d_out = c->d_counts;
    if (!c->d_patterns || c->n_pat == 0) return fail(KMPGPU_ESTATE, "kmpgpu_scan: no patterns set");
    if (!c->d_off && c->n_pkts) return fail(KMPGPU_ESTATE, "kmpgpu_scan: no arena loaded");
    uint32_t nl = 0;
    if (c->n_pkts == 0) {
        if (!accumulate) HIP_TRY(hipMemsetAsync(d_out, 0, sizeof(unsigned long long) * c->n_pat, c->stream));
        if (launches) *launches = 0;
        return KMPGPU_OK;
    }
    /* the folded copy first: a failure leaves no pass half enqueued */
    int rc = c->sets[1].n ? ensure_fold(c) : KMPGPU_OK;
    if (rc) return rc;
    /* the grid depends on the set (the fused pass); the partials are sized for the larger of the two passes, which run one after the
     * other on the stream and reuse them */
    uint32_t bx[2] = {0, 0};
    size_t elems = 0;
    for (int k = 0; k < 2; k++)
        if (c->sets[k].n) {
            bx[k] = grid_blocks(c, c->sets[k], emit != nullptr);
            elems = std::max(elems, (size_t)bx[k] * part_rows(c, c->sets[k]));
        }
    HIP_TRY(grow_buffer(&c->d_partials, &c->partials_cap, elems, EXACT));
    for (int k = 0; k < 2; k++)
        if (c->sets[k].n && (rc = enqueue_set(c, c->sets[k], k ? c->d_fold : c->d_arena, bx[k], nl, d_out, accumulate, emit))) return rc;
    if (launches) *launches = nl;
    return KMPGPU_OK;
}

hipError_t upload_words(uint32_t **d, const std::vector<uint32_t> &v)
{
    hipError_t e = hipMalloc(d, (v.size() ? v.size() : 1) * sizeof(uint32_t));
    if (e == hipSuccess && !v.empty()) e = hipMemcpy(*d, v.data(), v.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
    return e;
}

/* The passes of one set (kmpgpu_ctx::PatternSet) over the patterns `members` (indices into host, file order): the long / short split
 * of the streaming passes and the tables of the fused pass as kmp_build_tables makes them (kmp_tables.cpp), uploaded. */
int build_set(kmpgpu_ctx::PatternSet &s, const std::vector<kmp_pattern_dev> &host, const std::vector<uint32_t> &members)
{
    s.n = (uint32_t)members.size();
    if (!s.n) return KMPGPU_OK;
    kmp_set_tables t;
    if (!kmp_build_tables(host.data(), members, &t)) return fail(KMPGPU_EINVAL, "kmpgpu_set_patterns: fused tables: entry list overflow");
    s.n_long = t.n_long; s.n_short = t.n_short;
    HIP_TRY(upload_words(&s.d_ids, t.ids));
    for (const kmp_group_tables &h : t.groups) {
        s.fused_groups.emplace_back();
        kmpgpu_ctx::FusedGroup &g = s.fused_groups.back();
        HIP_TRY(upload_words(&g.d_tables, h.tables));
        HIP_TRY(upload_words(&g.d_ids, h.ids));
        HIP_TRY(upload_words(&g.d_rows, h.rows));
        HIP_TRY(upload_words(&g.d_uid_first, h.uid_first));
        HIP_TRY(upload_words(&g.d_uid_ids, h.uid_ids));
        g.words = (uint32_t)h.tables.size(); g.n_ids = (uint32_t)h.ids.size();
        g.n_unique = h.n_unique; g.cshift = h.cshift; g.classed = h.classed; g.bmask = h.bmask; g.n_ones = h.n_ones; g.ones = h.ones;
    }
    s.n_multi_unique = t.n_multi_unique;
    if (t.groups.empty()) return KMPGPU_OK;           /* nothing to fuse: every pattern keeps its own pass (s.d_ids) */
    HIP_TRY(upload_words(&s.d_rest_ids, t.rest));
    s.rest_long = t.rest_long; s.rest_short = t.rest_short;
    return KMPGPU_OK;
}

}  // namespace

extern "C" {

const char *kmpgpu_last_error(void) { return g_err.c_str(); }

int kmpgpu_device_count(void)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return fail(KMPGPU_EHIP, "hipGetDeviceCount failed: %s", hipGetErrorString(e));
    return n;
}

int kmpgpu_init(kmpgpu_ctx **out, int device)
{
    if (!out) return fail(KMPGPU_EINVAL, "kmpgpu_init: ctx is NULL");
    *out = nullptr;
    int n = 0;
    HIP_TRY(hipGetDeviceCount(&n));
    if (n <= 0) return fail(KMPGPU_EHIP, "kmpgpu_init: no HIP device visible");
    if (device < 0 || device >= n) return fail(KMPGPU_EINVAL, "kmpgpu_init: device %d out of range (0..%d)", device, n - 1);
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(KMPGPU_EHIP, "kmpgpu_init: device %d is %s; this library carries gfx950 code only", device, prop.gcnArchName);
    kmpgpu_ctx *c = new (std::nothrow) kmpgpu_ctx();
    if (!c) return fail(KMPGPU_ENOMEM, "kmpgpu_init: out of host memory");
    c->device = device;
    c->id = ++g_ctx_ids;
    c->cu_count = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    hipError_t e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking);
    if (e == hipSuccess) {
        c->stream = c->own_stream;
        for (auto &ev : c->ev) if (e == hipSuccess) e = hipEventCreate(&ev);
    }
    if (e == hipSuccess) e = hipMalloc(&c->d_err, 2 * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc(&c->d_sum, 6 * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipHostMalloc((void **)&c->h_small, 16 * sizeof(unsigned long long), hipHostMallocDefault);
    if (e != hipSuccess) {
        kmpgpu_destroy(c);
        return fail(KMPGPU_EHIP, "kmpgpu_init: %s", hipGetErrorString(e));
    }
    *out = c;
    return KMPGPU_OK;
}

void kmpgpu_destroy(kmpgpu_ctx *c)
{
    if (!c) return;
    if (c->comm) comm_forget(c->comm, c);           /* a communicator outliving one of its contexts: it keeps device + stream handle only */
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    release_arena(c);
    release_frame_scratch(c);
    release_pass_buffers(c);
    release_patterns(c);
    free_buffer(&c->d_err);                         /* (what kmpgpu_init took) */
    free_buffer(&c->d_sum);
    if (c->h_counts) (void)hipHostFree(c->h_counts);
    if (c->h_small) (void)hipHostFree(c->h_small);
    for (auto ev : c->ev) if (ev) (void)hipEventDestroy(ev);
    for (auto ev : c->prof_ev) if (ev) (void)hipEventDestroy(ev);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
}

int kmpgpu_set_stream(kmpgpu_ctx *c, void *hip_stream)
{
    if (!c) return fail(KMPGPU_EINVAL, "kmpgpu_set_stream: ctx is NULL");
    c->stream = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
    return KMPGPU_OK;
}

int kmpgpu_set_option(kmpgpu_ctx *c, int key, int64_t value)
{
    if (!c) return fail(KMPGPU_EINVAL, "kmpgpu_set_option: ctx is NULL");
    switch (key) {
    case KMPGPU_OPT_MODE:
        if (value != 0 && value != 1) return fail(KMPGPU_EINVAL, "mode must be 0 or 1");
        c->mode = (int)value; return KMPGPU_OK;
    case KMPGPU_OPT_BLOCKS_PER_CU:
        if (value < 0 || value > 256) return fail(KMPGPU_EINVAL, "blocks per CU must be 0 (auto) or 1..256");
        c->blocks_per_cu = (int)value; return KMPGPU_OK;
    case KMPGPU_OPT_DEPTH:
        if (value != 0 && (value < 2 || value > 8 || value == 7)) return fail(KMPGPU_EINVAL, "depth must be 0 (auto), 2..6 or 8");
        c->depth = (int)value; return KMPGPU_OK;
    case KMPGPU_OPT_FUSED:
        if (value < 0 || value > 2) return fail(KMPGPU_EINVAL, "fused must be 0, 1 or 2");
        c->fused = (int)value; return KMPGPU_OK;
    case KMPGPU_OPT_REPACK:
        c->repack = value ? 1 : 0; return KMPGPU_OK;
    case KMPGPU_OPT_ACCUMULATE:
        c->accumulate = value ? 1 : 0; return KMPGPU_OK;
    case KMPGPU_OPT_KERNEL:
        if (value < 0 || value > 3) return fail(KMPGPU_EINVAL, "kernel selection must be 0, 1, 2 or 3");
        c->kernel_sel = (int)value; return KMPGPU_OK;
    case KMPGPU_OPT_NONTEMPORAL:
        c->nontemporal = value ? 1 : 0; return KMPGPU_OK;
    case KMPGPU_OPT_FUSED_UNIT:
        if (value != 0 && (value < 1024 || value > (1 << 20) || (value & 1023))) return fail(KMPGPU_EINVAL, "fused unit must be 0 (auto) or a multiple of 1024 up to 1 MiB");
        c->fused_unit = (int)value; return KMPGPU_OK;
    case KMPGPU_OPT_WHOLE_PAYLOAD:
        if (value != 0 && value != 1) return fail(KMPGPU_EINVAL, "whole payload must be 0 (text ends at a payload's first 0x00) or 1 (at its end)");
        c->whole_payload = (int)value; return KMPGPU_OK;
    case KMPGPU_OPT_KEEP_META:
        if (value != 0 && value != 1) return fail(KMPGPU_EINVAL, "keep meta must be 0 (kmpgpu_load_frames builds the arena alone) or 1 (and keeps the payloads' header metadata)");
        c->keep_meta = (int)value; return KMPGPU_OK;
    case KMPGPU_OPT_FLOW_SLOTS:
        if (value < 0) return fail(KMPGPU_EINVAL, "flow slots must be 0 (auto) or a power of two above the payload count");
        c->flow_slots = value; return KMPGPU_OK;
    default:
        return fail(KMPGPU_EINVAL, "unknown option %d", key);
    }
}

void *kmpgpu_host_alloc(size_t bytes)
{
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) {
        fail(KMPGPU_EHIP, "hipHostMalloc(%zu) failed", bytes);
        return nullptr;
    }
    return p;
}

void kmpgpu_host_free(void *p) { if (p) (void)hipHostFree(p); }

int kmpgpu_host_register(const void *ptr, size_t bytes)
{
    if (!ptr || !bytes) return fail(KMPGPU_EINVAL, "kmpgpu_host_register: NULL / empty range");
    if ((uintptr_t)ptr & 4095u) return fail(KMPGPU_EINVAL, "kmpgpu_host_register: the range must start on a page boundary");
    /* portable: visible to every device's context (several shards upload from one mapping); the memory may be a PROT_READ mapping */
    hipError_t e = hipHostRegister(const_cast<void *>(ptr), bytes, hipHostRegisterPortable | hipHostRegisterReadOnly);
    if (e != hipSuccess) { (void)hipGetLastError(); e = hipHostRegister(const_cast<void *>(ptr), bytes, hipHostRegisterPortable); }
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(KMPGPU_EHIP, "hipHostRegister(%zu bytes) failed: %s", bytes, hipGetErrorString(e)); }
    std::lock_guard<std::mutex> lock(g_pinned_mu);
    g_pinned[(uintptr_t)ptr] = bytes;
    return KMPGPU_OK;
}

int kmpgpu_host_unregister(const void *ptr)
{
    if (!ptr) return fail(KMPGPU_EINVAL, "kmpgpu_host_unregister: NULL");
    { std::lock_guard<std::mutex> lock(g_pinned_mu); g_pinned.erase((uintptr_t)ptr); }
    HIP_TRY(hipHostUnregister(const_cast<void *>(ptr)));
    return KMPGPU_OK;
}

int kmpgpu_set_patterns(kmpgpu_ctx *c, const uint8_t *const *pat, const uint32_t *pat_len, uint32_t n_pat)
{
    return kmpgpu_set_patterns_flags(c, pat, pat_len, nullptr, n_pat);
}

int kmpgpu_set_patterns_flags(kmpgpu_ctx *c, const uint8_t *const *pat, const uint32_t *pat_len, const uint32_t *flags, uint32_t n_pat)
{
    if (!c) return fail(KMPGPU_EINVAL, "kmpgpu_set_patterns: ctx is NULL");
    if (n_pat && (!pat || !pat_len)) return fail(KMPGPU_EINVAL, "kmpgpu_set_patterns: NULL pattern arrays");
    HIP_TRY(hipSetDevice(c->device));
    std::vector<kmp_pattern_dev> host(n_pat ? n_pat : 1);
    std::vector<uint32_t> members[2];              /* the patterns of sets[0] (case-sensitive) and sets[1] (nocase, with a letter) */
    for (uint32_t i = 0; i < n_pat; i++) {
        const uint32_t m = pat_len[i];
        if (m < 1 || m > KMPGPU_MAX_PATTERN_LEN) return fail(KMPGPU_EINVAL, "pattern %u: length %u not in 1..99", i, m);
        if (!pat[i]) return fail(KMPGPU_EINVAL, "pattern %u is NULL", i);
        if (memchr(pat[i], 0, m)) return fail(KMPGPU_EINVAL, "pattern %u contains a 0x00 byte", i);
        const uint32_t fl = flags ? flags[i] : 0u;
        if (fl & ~KMPGPU_PAT_NOCASE) return fail(KMPGPU_EINVAL, "pattern %u: unknown flag bits 0x%x", i, fl & ~KMPGPU_PAT_NOCASE);
        kmp_pattern_dev &d = host[i];
        memset(&d, 0, sizeof d);
        memcpy(d.pat, pat[i], m);
        /* nocase: stored folded (ASCII A-Z -> a-z, kmp_fold.hip), failure table included; without a letter it is its case-sensitive self */
        bool letter = false;
        if (fl & KMPGPU_PAT_NOCASE)
            for (uint32_t b = 0; b < m; b++) {
                if (d.pat[b] >= 'A' && d.pat[b] <= 'Z') d.pat[b] += 'a' - 'A';
                letter |= d.pat[b] >= 'a' && d.pat[b] <= 'z';
            }
        failure_table(d.pat, m, d.fail);
        d.m = m;
        const uint32_t f = m < 4 ? m : 4;
        for (uint32_t b = 0; b < f; b++) { d.first |= (uint32_t)d.pat[b] << (8 * b); d.mask |= 0xFFu << (8 * b); }
        members[letter ? 1 : 0].push_back(i);
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    release_patterns(c);
    c->n_pat = n_pat;
    for (uint32_t i = 0; i < n_pat; i++) {
        c->pat_sig.push_back((uint8_t)pat_len[i]);
        c->pat_sig.push_back((uint8_t)(flags ? flags[i] : 0u));
        c->pat_sig.insert(c->pat_sig.end(), pat[i], pat[i] + pat_len[i]);
    }
    c->pat_fold.assign(n_pat, 0);
    for (uint32_t i : members[1]) c->pat_fold[i] = 1;
    const size_t np = n_pat ? n_pat : 1;
    HIP_TRY(hipMalloc(&c->d_patterns, np * sizeof(kmp_pattern_dev)));
    HIP_TRY(hipMalloc(&c->d_counts, np * sizeof(unsigned long long)));
    HIP_TRY(hipMemset(c->d_counts, 0, np * sizeof(unsigned long long)));
    if (n_pat) HIP_TRY(hipMemcpy(c->d_patterns, host.data(), n_pat * sizeof(kmp_pattern_dev), hipMemcpyHostToDevice));
    if (c->h_counts_cap < np) {
        if (c->h_counts) (void)hipHostFree(c->h_counts);
        c->h_counts = nullptr; c->h_counts_cap = 0;
        HIP_TRY(hipHostMalloc((void **)&c->h_counts, np * sizeof(uint64_t), hipHostMallocDefault));
        c->h_counts_cap = np;
    }
    for (int k = 0; k < 2; k++) {
        const int rc = build_set(c->sets[k], host, members[k]);
        if (rc) return rc;
    }
    /* an arena is attached already: its fold buffer now (a failure is reported by the first scan that needs the buffer) */
    if (c->n_pkts) (void)grow_fold(c, c->arena_bytes);
    return KMPGPU_OK;
}

int kmpgpu_load_arena(kmpgpu_ctx *c, const uint8_t *arena, uint64_t arena_bytes, const uint64_t *pkt_off,
                      const uint32_t *pkt_len, uint64_t n_pkts)
{
    if (!c) return fail(KMPGPU_EINVAL, "kmpgpu_load_arena: ctx is NULL");
    if (n_pkts && (!arena || !pkt_off || !pkt_len)) return fail(KMPGPU_EINVAL, "kmpgpu_load_arena: NULL buffers");
    IndexFacts f;
    for (uint64_t k = 0; k < n_pkts; k++) {         /* the layout contract the kernels rely on */
        const uint64_t o = pkt_off[k], l16 = ((uint64_t)pkt_len[k] + 15u) & ~15ull;
        if (o & 15u) return fail(KMPGPU_EINVAL, "payload %llu: offset %llu is not 16-byte aligned", (unsigned long long)k, (unsigned long long)o);
        if (pkt_len[k] > (1u << 30)) return fail(KMPGPU_EINVAL, "payload %llu: length %u is above 2^30", (unsigned long long)k, pkt_len[k]);
        if (o > arena_bytes || std::max<uint64_t>(l16, 16) > arena_bytes - o)
            return fail(KMPGPU_EINVAL, "payload %llu: [%llu, +%llu) padded to 16 B (at least one 16-byte slot) exceeds the arena (%llu B)", (unsigned long long)k,
                        (unsigned long long)o, (unsigned long long)pkt_len[k], (unsigned long long)arena_bytes);
        f.payload_bytes += pkt_len[k];
        f.span_end = o + std::max<uint64_t>(l16, 16);
        f.fold_end = std::max<uint64_t>(f.fold_end, f.span_end);
    }
    f.packed = n_pkts > 0;
    for (uint64_t k = 0; f.packed && k + 1 < n_pkts; k++)
        if (pkt_off[k + 1] != pkt_off[k] + std::max<uint64_t>(((uint64_t)pkt_len[k] + 15u) & ~15ull, 16)) f.packed = false;
    f.uniform = n_pkts > 0;
    if (f.uniform) {
        const uint64_t l16 = std::max<uint64_t>(((uint64_t)pkt_len[0] + 15u) & ~15ull, 16);
        const uint64_t ustride = n_pkts > 1 ? pkt_off[1] - pkt_off[0] : l16;
        if (n_pkts > 1 && pkt_off[1] < pkt_off[0]) f.uniform = false;
        if (ustride < l16 || (ustride & 15u) || ustride >= (1ull << 31)) f.uniform = false;
        for (uint64_t k = 0; f.uniform && k < n_pkts; k++)
            if (pkt_len[k] != pkt_len[0] || pkt_off[k] != pkt_off[0] + k * ustride) f.uniform = false;
        f.off0 = pkt_off[0]; f.stride = (uint32_t)ustride; f.len0 = pkt_len[0];
    }
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    /* streamed captures load batch after batch: keep the device buffers when the next batch fits */
    const bool reuse = owned_arena_holds(c, arena_bytes, n_pkts) && n_pkts > 0;
    release_arena(c, reuse);
    c->last.h2d_ms = 0; c->last.h2d_bytes = 0;
    if (n_pkts == 0) return KMPGPU_OK;
    if (arena_bytes < 16) return fail(KMPGPU_EINVAL, "arena smaller than 16 bytes");
    HIP_TRY(ensure_owned_arena(c, arena_bytes, n_pkts, EXACT));
    HIP_TRY(hipEventRecord(c->ev[0], c->stream));
    HIP_TRY(upload_split(c->owned_arena, arena, arena_bytes, c->stream));
    HIP_TRY(hipMemcpyAsync(c->owned_off, pkt_off, n_pkts * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->owned_len, pkt_len, n_pkts * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipEventRecord(c->ev[1], c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    c->last.h2d_ms = ms;
    c->last.h2d_bytes = arena_bytes + n_pkts * (sizeof(uint64_t) + sizeof(uint32_t));
    return install_arena(c, c->owned_arena, c->owned_off, c->owned_len, arena_bytes, n_pkts, f, /* wrote_padding = */ false);
}

int kmpgpu_load_frames_begin(kmpgpu_ctx *c, const uint8_t *file_bytes, uint64_t file_nbytes, const uint64_t *frame_off,
                             const uint32_t *frame_caplen, uint64_t n_frames, int tcp)
{
    if (!c) return fail(KMPGPU_EINVAL, "kmpgpu_load_frames: ctx is NULL");
    if (n_frames && (!file_bytes || !frame_off || !frame_caplen)) return fail(KMPGPU_EINVAL, "kmpgpu_load_frames: NULL buffers");
    if (c->fr_pending) return fail(KMPGPU_ESTATE, "kmpgpu_load_frames_begin: the previous load has not been finished");
    /* Only the bytes these frames span are uploaded: a shard of the frames (mpi_dumping.c:149-161 scatters shares, not
     * the whole capture) or a batch of a streamed capture (openmp_task.c:126-155) costs its share of PCIe time and HBM. */
    uint64_t span_lo = file_nbytes, span_hi = 0;
    for (uint64_t f = 0; f < n_frames; f++) {
        if (frame_off[f] > file_nbytes || frame_caplen[f] > file_nbytes - frame_off[f])
            return fail(KMPGPU_EINVAL, "kmpgpu_load_frames: frame %llu lies outside the file buffer", (unsigned long long)f);
        span_lo = std::min<uint64_t>(span_lo, frame_off[f]);
        span_hi = std::max<uint64_t>(span_hi, frame_off[f] + frame_caplen[f]);
    }
    if (span_hi < span_lo) span_lo = span_hi = 0;
    span_lo &= ~(uint64_t)15;                           /* keeps the frames' alignment relative to the device buffer */
    const uint64_t span = span_hi - span_lo;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));           /* the passes over the arena that is about to be replaced */
    release_arena(c, /* keep_buffers = */ true);        /* batch after batch: device buffers are reused when the next batch fits */
    c->last.h2d_ms = 0; c->last.h2d_bytes = 0;
    c->fr_pending = true; c->fr_n = n_frames; c->fr_tcp = tcp; c->fr_span = span; c->fr_span_lo = span_lo;
    c->fr_meta = c->keep_meta != 0;
    if (n_frames == 0) return KMPGPU_OK;

    /* scratch, grown on demand and kept (no hipMalloc / hipFree per batch: either synchronises the whole device) */
    HIP_TRY(grow_buffer(&c->fr_file, &c->fr_file_cap, span + 64, EIGHTH));
    HIP_TRY(grow_buffer(&c->fr_off, &c->fr_off_cap, n_frames, EIGHTH));
    HIP_TRY(grow_buffer(&c->fr_cl, &c->fr_cl_cap, n_frames, EIGHTH));
    HIP_TRY(grow_buffer(&c->fr_ws, &c->fr_ws_cap, (uint64_t)kmp_extract_ws_bytes(n_frames), EIGHTH));
    if (!c->fr_tot) HIP_TRY(hipMalloc(&c->fr_tot, 2 * sizeof(unsigned long long)));

    /* the device buffer holds the file's bytes [span_lo, span_hi): the kernels address it through the pointer that stands for
     * the file's first byte, so the frame offsets go up as they are (no rebased copy of them on the host) */
    const uint8_t *d_file0 = c->fr_file - span_lo;
    HIP_TRY(hipEventRecord(c->ev[0], c->stream));
    HIP_TRY(upload_split(c->fr_file, file_bytes + span_lo, span, c->stream));
    HIP_TRY(hipMemcpyAsync(c->fr_off, frame_off, n_frames * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->fr_cl, frame_caplen, n_frames * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipEventRecord(c->ev[1], c->stream));
    HIP_TRY(kmp_launch_extract_phase1(d_file0, c->fr_off, c->fr_cl, n_frames, tcp, c->fr_ws, c->fr_tot, c->stream));
    HIP_TRY(hipMemcpyAsync(c->h_small, c->fr_tot, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));         /* (pinned: no staging) */
    return KMPGPU_OK;
}

int kmpgpu_load_frames_uploaded(kmpgpu_ctx *c)
{
    if (!c) return fail(KMPGPU_EINVAL, "kmpgpu_load_frames_uploaded: ctx is NULL");
    if (!c->fr_pending || c->fr_n == 0) return KMPGPU_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipEventSynchronize(c->ev[1]));
    return KMPGPU_OK;
}

int kmpgpu_load_frames_finish(kmpgpu_ctx *c, uint64_t *n_payloads)
{
    if (!c) return fail(KMPGPU_EINVAL, "kmpgpu_load_frames: ctx is NULL");
    if (n_payloads) *n_payloads = 0;
    if (!c->fr_pending) return fail(KMPGPU_ESTATE, "kmpgpu_load_frames_finish: no load has been begun");
    c->fr_pending = false;
    const uint64_t n_frames = c->fr_n, span = c->fr_span;
    if (n_frames == 0) return KMPGPU_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    unsigned long long tot[2] = {0, 0};
    memcpy(tot, c->h_small, sizeof tot);
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    c->last.h2d_ms = ms;
    c->last.h2d_bytes = span + n_frames * (sizeof(uint64_t) + sizeof(uint32_t));
    const uint64_t n_pkts = tot[1], arena_bytes = tot[0] + 64;
    if (n_payloads) *n_payloads = n_pkts;
    if (n_pkts == 0) return KMPGPU_OK;
    HIP_TRY(ensure_owned_arena(c, arena_bytes, n_pkts, EIGHTH));
    HIP_TRY(grow_buffer(&c->fr_src, &c->fr_src_cap, n_pkts, EIGHTH));
    if (c->fr_meta) HIP_TRY(grow_buffer(&c->d_meta, &c->meta_cap, n_pkts, EIGHTH));
    const uint8_t *d_file0 = c->fr_file - c->fr_span_lo;
    HIP_TRY(hipMemsetAsync(c->owned_arena + tot[0], 0, 64, c->stream));
    HIP_TRY(kmp_launch_extract_phase2(d_file0, c->fr_off, n_frames, c->fr_ws, n_pkts, c->owned_arena, c->owned_off, c->owned_len, c->fr_src, c->stream));
    /* KMPGPU_OPT_KEEP_META: the accepted frames' header fields, by the numbering the scatter has just used */
    if (c->fr_meta) HIP_TRY(kmp_launch_meta_extract(d_file0, c->fr_off, n_frames, c->fr_ws, c->d_meta, c->stream));
    IndexFacts f;
    int rc = validate_index(c, "kmpgpu_load_frames", c->owned_off, c->owned_len, n_pkts, arena_bytes, &f);
    /* kmp_gather_kernel writes every slot whole: payload, then 0x00 up to the slot's end */
    if (!rc) rc = install_arena(c, c->owned_arena, c->owned_off, c->owned_len, arena_bytes, n_pkts, f, /* wrote_padding = */ true);
    if (!rc) c->has_meta = c->fr_meta;
    /* one capture uploaded whole: its bytes are not kept around (a streamed capture's batches are small and the next one
     * reuses the buffer) */
    if (c->fr_file_cap > (1ull << 30)) free_buffer(&c->fr_file, &c->fr_file_cap);
    return rc;
}

int kmpgpu_load_frames(kmpgpu_ctx *c, const uint8_t *file_bytes, uint64_t file_nbytes, const uint64_t *frame_off,
                       const uint32_t *frame_caplen, uint64_t n_frames, int tcp, uint64_t *n_payloads)
{
    if (n_payloads) *n_payloads = 0;
    const int rc = kmpgpu_load_frames_begin(c, file_bytes, file_nbytes, frame_off, frame_caplen, n_frames, tcp);
    return rc ? rc : kmpgpu_load_frames_finish(c, n_payloads);
}

int kmpgpu_reserve(kmpgpu_ctx *c, uint64_t arena_bytes, uint64_t n_pkts, uint64_t frame_bytes, uint64_t n_frames)
{
    if (!c) return fail(KMPGPU_EINVAL, "kmpgpu_reserve: ctx is NULL");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (arena_bytes && n_pkts && !owned_arena_holds(c, arena_bytes, n_pkts)) {
        if (c->d_arena == c->owned_arena) release_arena(c, true);        /* the arena in use lives in these buffers */
        HIP_TRY(ensure_owned_arena(c, arena_bytes, n_pkts, EXACT));
    }
    if (arena_bytes) {
        const uint64_t words = arena_bytes / KMP_CHUNK + 32;
        if (c->bitmap_cap < words && c->bitmap_live) return fail(KMPGPU_ESTATE, "kmpgpu_reserve: an arena larger than the reserved size is attached");
        HIP_TRY(grow_buffer(&c->d_bitmap, &c->bitmap_cap, words, EXACT));
        const int rc = grow_fold(c, arena_bytes);    /* the nocase patterns' folded copy of a batch */
        if (rc) return rc;
    }
    if (frame_bytes && n_frames) {
        HIP_TRY(grow_buffer(&c->fr_file, &c->fr_file_cap, frame_bytes + 64, EIGHTH));
        HIP_TRY(grow_buffer(&c->fr_off, &c->fr_off_cap, n_frames, EIGHTH));
        HIP_TRY(grow_buffer(&c->fr_cl, &c->fr_cl_cap, n_frames, EIGHTH));
        HIP_TRY(grow_buffer(&c->fr_ws, &c->fr_ws_cap, (uint64_t)kmp_extract_ws_bytes(n_frames), EIGHTH));
        HIP_TRY(grow_buffer(&c->fr_src, &c->fr_src_cap, n_frames, EIGHTH));
        if (!c->fr_tot) HIP_TRY(hipMalloc(&c->fr_tot, 2 * sizeof(unsigned long long)));
        HIP_TRY(hipMemsetAsync(c->fr_file, 0, frame_bytes + 64, c->stream));      /* first touch now: the first upload into fresh device memory runs at 3/4 of the rate */
    }
    if (c->owned_arena && arena_bytes && c->d_arena != c->owned_arena) HIP_TRY(hipMemsetAsync(c->owned_arena, 0, std::min<uint64_t>(arena_bytes, c->cap_arena), c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return KMPGPU_OK;
}

int kmpgpu_attach_arena(kmpgpu_ctx *c, const void *d_arena, uint64_t arena_bytes, const void *d_pkt_off,
                        const void *d_pkt_len, uint64_t n_pkts)
{
    if (!c) return fail(KMPGPU_EINVAL, "kmpgpu_attach_arena: ctx is NULL");
    if (n_pkts && (!d_arena || !d_pkt_off || !d_pkt_len)) return fail(KMPGPU_EINVAL, "kmpgpu_attach_arena: NULL buffers");
    if (((uintptr_t)d_arena & 15u) || ((uintptr_t)d_pkt_off & 7u) || ((uintptr_t)d_pkt_len & 3u))
        return fail(KMPGPU_EINVAL, "kmpgpu_attach_arena: misaligned device pointer");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    release_arena(c);
    if (n_pkts == 0) return KMPGPU_OK;
    if (arena_bytes < 16) return fail(KMPGPU_EINVAL, "arena smaller than 16 bytes");
    IndexFacts f;
    const int rc = validate_index(c, "kmpgpu_attach_arena", (const uint64_t *)d_pkt_off, (const uint32_t *)d_pkt_len, n_pkts, arena_bytes, &f);
    if (rc) return rc;                               /* (nothing is attached) */
    return install_arena(c, (const uint8_t *)d_arena, (const uint64_t *)d_pkt_off, (const uint32_t *)d_pkt_len, arena_bytes, n_pkts, f, /* wrote_padding = */ false);
}

int kmpgpu_load_selected(kmpgpu_ctx *dst, kmpgpu_ctx *src, const void *select, int select_on_device, uint64_t *n_selected)
{
    const char *who = "kmpgpu_load_selected";
    if (n_selected) *n_selected = 0;
    if (const int rc = pair_refused(dst, src, who)) return rc;
    if (select_on_device != 0 && select_on_device != 1) return fail(KMPGPU_EINVAL, "%s: select_on_device is %d, not 0 or 1", who, select_on_device);
    if (const int rc = pair_state_refused(dst, src, who, "selection")) return rc;
    const uint64_t n = src->n_pkts;
    if (n && !select) return fail(KMPGPU_EINVAL, "%s: select is NULL", who);
    if (n && select_on_device && ((uintptr_t)select & 7u)) return fail(KMPGPU_EINVAL, "%s: the device bitmap is not 8-byte aligned", who);
    if (const int rc = derived_begin(dst, src)) return rc;
    kmpgpu_ctx *c = dst;
    if (n == 0) { release_arena(c, /* keep_buffers = */ true); return KMPGPU_OK; }

    /* the scratch of kmpgpu_load_frames: fr_off takes the uploaded bitmap, fr_ws the scan, fr_src the copy's records */
    const uint64_t words = (n + 63) / 64;
    HIP_TRY(grow_buffer(&c->fr_ws, &c->fr_ws_cap, (uint64_t)kmp_extract_ws_bytes(n), EIGHTH));
    if (!c->fr_tot) HIP_TRY(hipMalloc(&c->fr_tot, 2 * sizeof(unsigned long long)));
    const unsigned long long *d_select = (const unsigned long long *)select;
    if (!select_on_device) {
        HIP_TRY(grow_buffer(&c->fr_off, &c->fr_off_cap, words, EIGHTH));
        HIP_TRY(hipEventRecord(c->ev[0], c->stream));
        HIP_TRY(hipMemcpyAsync(c->fr_off, select, words * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipEventRecord(c->ev[1], c->stream));
        d_select = (const unsigned long long *)c->fr_off;
    }
    HIP_TRY(hipEventRecord(c->ev[2], c->stream));
    HIP_TRY(kmp_launch_select_phase1(d_select, src->d_len, n, c->fr_ws, c->fr_tot, c->stream));
    unsigned long long tot[2] = {0, 0};
    if (const int rc = read_totals(c, tot)) return rc;
    if (!select_on_device) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
        c->last.h2d_ms = ms; c->last.h2d_bytes = words * sizeof(uint64_t);
    }
    const uint64_t n_pkts = tot[1];
    const uint32_t meta_launch = src->has_meta ? 1u : 0u;
    /* from here on dst's earlier arena is gone, whatever happens */
    release_arena(c, /* keep_buffers = */ true);
    if (n_pkts == 0) {
        if (src->has_meta) HIP_TRY(kmp_launch_meta_select(src->d_meta, n, c->fr_ws, c->d_meta, c->stream));       /* (finds no record to move) */
        return derived_finish(c, 3 + meta_launch, /* record = */ true);
    }
    if (const int rc = take_arena(c, who, tot[0], n_pkts, "payloads")) return rc;
    hipError_t e = grow_buffer(&c->fr_src, &c->fr_src_cap, 2 * n_pkts, EIGHTH);      /* 16 bytes per selected payload */
    if (e != hipSuccess) return alloc_fail(e, "%s: the copy's records (%llu payloads) could not be allocated", who, (unsigned long long)n_pkts);
    if (src->has_meta) {
        e = grow_buffer(&c->d_meta, &c->meta_cap, n_pkts, EIGHTH);
        if (e != hipSuccess) return alloc_fail(e, "%s: the metadata (%llu payloads) could not be allocated", who, (unsigned long long)n_pkts);
    }
    HIP_TRY(kmp_launch_select_phase2(src->d_arena, src->d_off, n, c->fr_ws, n_pkts, tot[0], c->owned_arena, c->owned_off, c->owned_len, c->fr_src,
                                     c->nontemporal != 0, c->stream));
    /* src has metadata: the selected payloads' records go with them, in their new order */
    if (src->has_meta) HIP_TRY(kmp_launch_meta_select(src->d_meta, n, c->fr_ws, c->d_meta, c->stream));
    HIP_TRY(hipEventRecord(c->ev[3], c->stream));
    if (const int rc = install_owned(c, who, tot[0], n_pkts)) return rc;
    if (const int rc = derived_finish(c, 5 + meta_launch, /* record = */ false)) return rc;
    c->has_meta = src->has_meta;
    if (n_selected) *n_selected = n_pkts;
    return KMPGPU_OK;
}

/* Which spans a call means: the HTTP ones, the DNS ones for a prefix flag (KMPGPU_DNS_TCP_PREFIX or 0), or the TLS ones. */
enum SpanProto { SPANS_HTTP, SPANS_DNS, SPANS_TLS };
struct SpanKind { SpanProto proto; uint32_t prefix; };
/* ... and where the context keeps them.  masks: 32 bytes of separator mask per payload stand behind the records */
struct SpanStore { uint4 **d; uint64_t *cap; uint64_t *stats; bool *valid; bool masks; };
static SpanStore span_store(kmpgpu_ctx *c, SpanKind sk)
{
    if (sk.proto == SPANS_DNS) return SpanStore{&c->d_dns, &c->dns_cap, c->dns_stats, &c->dns_valid, true};
    if (sk.proto == SPANS_TLS) return SpanStore{&c->d_tls, &c->tls_cap, c->tls_stats, &c->tls_valid, true};
    return SpanStore{&c->d_spans, &c->spans_cap, c->http_stats, &c->spans_valid, false};
}
static bool spans_current(kmpgpu_ctx *c, SpanKind sk) { return *span_store(c, sk).valid && (sk.proto != SPANS_DNS || c->dns_prefix == sk.prefix); }

/* The spans of src's arena, made on the stream of `on` (src itself, or the dst of kmpgpu_load_fields / kmpgpu_load_dns / kmpgpu_load_tls,
 * which has waited for src's stream) where they are stale; *launched: the kernel ran.  The caller synchronises the stream before it reads
 * the stats. */
static int locate_spans(kmpgpu_ctx *src, kmpgpu_ctx *on, SpanKind sk, const char *who, bool *launched)
{
    *launched = false;
    if (spans_current(src, sk)) return KMPGPU_OK;
    const uint64_t n = src->n_pkts;
    const SpanStore ss = span_store(src, sk);
    memset(ss.stats, 0, 4 * sizeof(uint64_t));
    *ss.valid = false;
    if (sk.proto == SPANS_DNS) src->dns_prefix = sk.prefix;
    if (n == 0) { *ss.valid = true; return KMPGPU_OK; }
    /* 32 bytes per payload, for DNS and TLS the separator masks of 32 bytes per payload behind them, 4 words of totals */
    const uint64_t units = ss.masks ? 4 * n : 2 * n;
    const hipError_t e = grow_buffer(ss.d, ss.cap, units + 2, EIGHTH);
    if (e != hipSuccess) return alloc_fail(e, "%s: the spans (%llu payloads) could not be allocated", who, (unsigned long long)n);
    uint4 *d = *ss.d;
    unsigned long long *d_stats = reinterpret_cast<unsigned long long *>(d + units);
    HIP_TRY(hipMemsetAsync(d_stats, 0, 4 * sizeof(unsigned long long), on->stream));
    HIP_TRY(profiled(on, [&] {
        if (sk.proto == SPANS_DNS) return kmp_launch_dns_locate(src->d_arena, src->d_off, src->d_len, n, sk.prefix != 0u, d, d + 2 * n, d_stats, on->stream);
        if (sk.proto == SPANS_TLS) return kmp_launch_tls_locate(src->d_arena, src->d_off, src->d_len, n, d, d + 2 * n, d_stats, on->stream);
        return kmp_launch_http_locate(src->d_arena, src->d_off, src->d_len, n, d, d_stats, on->stream);
    }));
    HIP_TRY(hipMemcpyAsync(on->h_small + 8, d_stats, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, on->stream));         /* (pinned: no staging) */
    *launched = true;
    return KMPGPU_OK;
}
/* ... and after that synchronisation */
static void located_spans(kmpgpu_ctx *src, kmpgpu_ctx *on, SpanKind sk)
{
    const SpanStore ss = span_store(src, sk);
    memcpy(ss.stats, on->h_small + 8, 4 * sizeof(uint64_t));
    *ss.valid = true;
}

/* kmpgpu_http_locate, kmpgpu_dns_locate and kmpgpu_tls_locate behind their own checks; the stats are then in c->http_stats / c->dns_stats /
 * c->tls_stats */
static int locate_call(kmpgpu_ctx *c, SpanKind sk, const char *who)
{
    if (c->fr_pending) return fail(KMPGPU_ESTATE, "%s: the context sits between kmpgpu_load_frames_begin and _finish", who);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->last = kmpgpu_timing{};
    bool launched = false;
    HIP_TRY(hipEventRecord(c->ev[2], c->stream));
    const int rc = locate_spans(c, c, sk, who, &launched);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(c->ev[3], c->stream));
    HIP_TRY(hipEventSynchronize(c->ev[3]));
    if (launched) {
        located_spans(c, c, sk);
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, c->ev[2], c->ev[3]));
        c->last.kernel_ms = ms; c->last.launches = 1;
    }
    return KMPGPU_OK;
}

int kmpgpu_http_locate(kmpgpu_ctx *c, kmpgpu_http_stats *stats)
{
    const char *who = "kmpgpu_http_locate";
    if (stats) *stats = kmpgpu_http_stats{};
    if (!c) return fail(KMPGPU_EINVAL, "%s: ctx is NULL", who);
    if (const int rc = locate_call(c, SpanKind{SPANS_HTTP, 0u}, who)) return rc;
    if (stats) { stats->n_requests = c->http_stats[0]; stats->n_responses = c->http_stats[1]; stats->n_blank = c->http_stats[2]; stats->bytes_scanned = c->http_stats[3]; }
    return KMPGPU_OK;
}

int kmpgpu_http_spans_read(kmpgpu_ctx *c, kmpgpu_http_span *out, uint64_t first, uint64_t n)
{
    const char *who = "kmpgpu_http_spans_read";
    static_assert(sizeof(kmpgpu_http_span) == 32, "kmpgpu_http_span is two 16-byte units");
    if (!c) return fail(KMPGPU_EINVAL, "%s: ctx is NULL", who);
    return read_range(c, who, c->spans_valid, "no spans (no kmpgpu_http_locate since the arena was set)", out, c->d_spans, 32, first, n, c->n_pkts, "records");
}

int kmpgpu_dns_locate(kmpgpu_ctx *c, uint32_t flags, kmpgpu_dns_stats *stats)
{
    const char *who = "kmpgpu_dns_locate";
    if (stats) *stats = kmpgpu_dns_stats{};
    if (!c) return fail(KMPGPU_EINVAL, "%s: ctx is NULL", who);
    if (flags & ~KMPGPU_DNS_TCP_PREFIX) return fail(KMPGPU_EINVAL, "%s: unknown flag bits 0x%x", who, flags);
    if (const int rc = locate_call(c, SpanKind{SPANS_DNS, flags}, who)) return rc;
    if (stats) { stats->n_queries = c->dns_stats[0]; stats->n_responses = c->dns_stats[1]; stats->n_root = c->dns_stats[2]; stats->name_bytes = c->dns_stats[3]; }
    return KMPGPU_OK;
}

int kmpgpu_dns_spans_read(kmpgpu_ctx *c, kmpgpu_dns_span *out, uint64_t first, uint64_t n)
{
    const char *who = "kmpgpu_dns_spans_read";
    static_assert(sizeof(kmpgpu_dns_span) == 32, "kmpgpu_dns_span is two 16-byte units");
    if (!c) return fail(KMPGPU_EINVAL, "%s: ctx is NULL", who);
    return read_range(c, who, c->dns_valid, "no spans (no kmpgpu_dns_locate since the arena was set)", out, c->d_dns, 32, first, n, c->n_pkts, "records");
}

int kmpgpu_tls_locate(kmpgpu_ctx *c, uint32_t flags, kmpgpu_tls_stats *stats)
{
    const char *who = "kmpgpu_tls_locate";
    if (stats) *stats = kmpgpu_tls_stats{};
    if (!c) return fail(KMPGPU_EINVAL, "%s: ctx is NULL", who);
    if (flags) return fail(KMPGPU_EINVAL, "%s: unknown flag bits 0x%x", who, flags);
    if (const int rc = locate_call(c, SpanKind{SPANS_TLS, 0u}, who)) return rc;
    if (stats) { stats->n_hellos = c->tls_stats[0]; stats->n_sni = c->tls_stats[1]; stats->n_alpn = c->tls_stats[2]; stats->n_truncated = c->tls_stats[3]; }
    return KMPGPU_OK;
}

int kmpgpu_tls_spans_read(kmpgpu_ctx *c, kmpgpu_tls_span *out, uint64_t first, uint64_t n)
{
    const char *who = "kmpgpu_tls_spans_read";
    static_assert(sizeof(kmpgpu_tls_span) == 32, "kmpgpu_tls_span is two 16-byte units");
    if (!c) return fail(KMPGPU_EINVAL, "%s: ctx is NULL", who);
    return read_range(c, who, c->tls_valid, "no spans (no kmpgpu_tls_locate since the arena was set)", out, c->d_tls, 32, first, n, c->n_pkts, "records");
}

/* What the five compacting loaders differ in: which lengths, index and write kernels run and what those take, whether src's spans are
 * located first, and whether dst holds only the payloads the bitmap marks (ONLY_CHANGED / ONLY_PRESENT). */
enum CompactKind { COMPACT_DECODE, COMPACT_BASE64, COMPACT_FIELDS, COMPACT_DNS, COMPACT_TLS };       /* from COMPACT_FIELDS on: over src's spans */
struct Compacting {
    const char *who;
    CompactKind kind;
    bool only_marked;
    bool plus, urlsafe;     /* KMPGPU_DECODE_PLUS; KMPGPU_B64_URLSAFE */
    uint32_t min_run;       /* base64 */
    int field;              /* fields, tls */
    SpanKind sk;            /* fields, dns, tls: the spans the kernels read */
};

/* The span the five calls share: the locate where the kernels read spans and src's are stale, lengths, scan, index, write.  st (zeroed by
 * the caller): the payloads dst holds, the set bits of the bitmap, the source bytes and the written bytes of the payloads dst holds. */
static int load_compacted(kmpgpu_ctx *dst, kmpgpu_ctx *src, const Compacting &how, uint64_t *bitmap_out, const void **d_bitmap, uint64_t st[4])
{
    const char *who = how.who;
    const bool spanned = how.kind >= COMPACT_FIELDS, only = how.only_marked;
    if (const int rc = derived_begin(dst, src)) return rc;
    kmpgpu_ctx *c = dst;
    const uint64_t n = src->n_pkts;
    if (n == 0) { release_arena(c, /* keep_buffers = */ true); return KMPGPU_OK; }

    /* the scratch of kmpgpu_load_frames (fr_ws the scan, fr_src the write's records) and the bitmap's own buffer, its four totals behind it */
    const uint64_t words = (n + 63) / 64;
    HIP_TRY(grow_buffer(&c->fr_ws, &c->fr_ws_cap, (uint64_t)kmp_extract_ws_bytes(n), EIGHTH));
    if (!c->fr_tot) HIP_TRY(hipMalloc(&c->fr_tot, 2 * sizeof(unsigned long long)));
    HIP_TRY(grow_buffer(&c->d_dec_changed, &c->dec_changed_cap, words + 4, EIGHTH));
    unsigned long long *bits = c->d_dec_changed, *d_stats = bits + words;
    HIP_TRY(hipMemsetAsync(d_stats, 0, 4 * sizeof(unsigned long long), c->stream));
    HIP_TRY(hipEventRecord(c->ev[2], c->stream));
    bool located = false;
    if (spanned)
        if (const int rc = locate_spans(src, c, how.sk, who, &located)) return rc;       /* (one more launch, where the spans are stale) */
    const uint4 *spans = spanned ? *span_store(src, how.sk).d : nullptr;
    const uint8_t *arena = src->d_arena;
    const uint64_t *off = src->d_off;
    const uint32_t *len = src->d_len;
    const bool nt = c->nontemporal != 0;
    HIP_TRY(profiled(c, [&] {
        switch (how.kind) {
        case COMPACT_DECODE: return kmp_launch_decode_lengths(arena, off, len, n, how.plus, only, c->fr_ws, bits, d_stats, c->stream);
        case COMPACT_BASE64: return kmp_launch_base64_lengths(arena, off, len, n, how.min_run, how.urlsafe, only, c->fr_ws, bits, d_stats, c->stream);
        case COMPACT_FIELDS: return kmp_launch_fields_lengths(spans, len, n, how.field, only, c->fr_ws, bits, d_stats, c->stream);
        case COMPACT_DNS: return kmp_launch_dns_lengths(spans, len, n, only, c->fr_ws, bits, d_stats, c->stream);
        default: return kmp_launch_tls_lengths(spans, len, n, how.field, only, c->fr_ws, bits, d_stats, c->stream);
        }
    }));
    HIP_TRY(profiled(c, [&] { return kmp_launch_compact_scan(n, c->fr_ws, c->fr_tot, c->stream); }));
    unsigned long long tot[6] = {0, 0, 0, 0, 0, 0};       /* packed bytes, payloads; source bytes, marked payloads, written bytes */
    if (const int rc = read_totals(c, tot, words, bitmap_out)) return rc;
    if (located) located_spans(src, c, how.sk);
    const uint64_t n_pkts = tot[1];
    auto done = [&](uint32_t launches, bool record) {
        if (const int rc = derived_finish(c, launches + (located ? 1u : 0u), record)) return rc;
        if (d_bitmap) *d_bitmap = bits;
        st[0] = n_pkts; st[1] = tot[3]; st[2] = tot[2]; st[3] = tot[4];
        return (int)KMPGPU_OK;
    };
    /* from here on dst's earlier arena is gone, whatever happens */
    release_arena(c, /* keep_buffers = */ true);
    if (n_pkts == 0) return done(3, /* record = */ true);
    if (const int rc = take_arena(c, who, tot[0], n_pkts, "payloads")) return rc;
    hipError_t e = grow_buffer(&c->fr_src, &c->fr_src_cap, 2 * n_pkts, EIGHTH);      /* 16 bytes per payload of dst */
    if (e != hipSuccess) return alloc_fail(e, "%s: the write's records (%llu payloads) could not be allocated", who, (unsigned long long)n_pkts);
    if (src->has_meta) {
        e = grow_buffer(&c->d_meta, &c->meta_cap, n_pkts, EIGHTH);
        if (e != hipSuccess) return alloc_fail(e, "%s: the metadata (%llu payloads) could not be allocated", who, (unsigned long long)n_pkts);
    }
    uint64_t *o_off = c->owned_off;
    uint32_t *o_len = c->owned_len;
    HIP_TRY(profiled(c, [&] {
        switch (how.kind) {
        case COMPACT_FIELDS: return kmp_launch_fields_index(spans, off, n, how.field, c->fr_ws, n_pkts, o_off, o_len, c->fr_src, c->stream);
        case COMPACT_DNS: return kmp_launch_dns_index(spans, off, n, c->fr_ws, n_pkts, o_off, o_len, c->fr_src, c->stream);
        case COMPACT_TLS: return kmp_launch_tls_index(spans, off, n, how.field, c->fr_ws, n_pkts, o_off, o_len, c->fr_src, c->stream);
        default: return kmp_launch_decode_index(off, len, n, c->fr_ws, n_pkts, o_off, o_len, c->fr_src, c->stream);
        }
    }));
    HIP_TRY(profiled(c, [&] {
        switch (how.kind) {
        case COMPACT_DECODE: return kmp_launch_decode_write(arena, o_off, c->fr_src, n_pkts, tot[2], tot[0], how.plus, c->owned_arena, nt, c->stream);
        case COMPACT_BASE64:
            return kmp_launch_base64_write(arena, o_off, c->fr_src, n_pkts, tot[2], tot[0], how.min_run, how.urlsafe, c->owned_arena, nt, c->stream);
        case COMPACT_FIELDS: return kmp_launch_fields_gather(arena, o_off, c->fr_src, n_pkts, tot[0], c->owned_arena, nt, c->stream);
        case COMPACT_DNS: return kmp_launch_dns_gather(arena, o_off, c->fr_src, spans + 2 * n, n_pkts, tot[0], c->owned_arena, nt, c->stream);
        default: return kmp_launch_tls_gather(arena, o_off, c->fr_src, spans + 2 * n, how.field, n_pkts, tot[0], c->owned_arena, nt, c->stream);
        }
    }));
    HIP_TRY(hipEventRecord(c->ev[3], c->stream));
    /* src has metadata: the records go with the payloads -- in their new order, or all of them as they are */
    if (src->has_meta) {
        if (only) HIP_TRY(kmp_launch_meta_select(src->d_meta, n, c->fr_ws, c->d_meta, c->stream));
        else HIP_TRY(hipMemcpyAsync(c->d_meta, src->d_meta, n * sizeof(uint4), hipMemcpyDeviceToDevice, c->stream));
    }
    if (const int rc = install_owned(c, who, tot[0], n_pkts)) return rc;
    c->has_meta = src->has_meta;
    return done(5, /* record = */ false);
}

/* kmpgpu_load_decoded and kmpgpu_load_base64 behind the checks of their own arguments */
static int recoded_call(kmpgpu_ctx *dst, kmpgpu_ctx *src, const Compacting &how, uint64_t *changed_out, const void **d_changed, kmpgpu_decode_stats *stats)
{
    if (const int rc = pair_state_refused(dst, src, how.who, "decoding")) return rc;
    uint64_t st[4] = {0, 0, 0, 0};
    const int rc = load_compacted(dst, src, how, changed_out, d_changed, st);
    if (!rc && stats) { stats->n_payloads = st[0]; stats->n_changed = st[1]; stats->bytes_in = st[2]; stats->bytes_out = st[3]; }
    return rc;
}

int kmpgpu_load_decoded(kmpgpu_ctx *dst, kmpgpu_ctx *src, int transform, uint32_t flags, uint64_t *changed_out, const void **d_changed,
                        kmpgpu_decode_stats *stats)
{
    const char *who = "kmpgpu_load_decoded";
    if (d_changed) *d_changed = nullptr;
    if (stats) *stats = kmpgpu_decode_stats{};
    if (const int rc = pair_refused(dst, src, who)) return rc;
    if (transform != KMPGPU_DECODE_PERCENT) return fail(KMPGPU_EINVAL, "%s: transform %d is not KMPGPU_DECODE_PERCENT", who, transform);
    if (flags & ~(KMPGPU_DECODE_PLUS | KMPGPU_DECODE_ONLY_CHANGED)) return fail(KMPGPU_EINVAL, "%s: unknown flag bits 0x%x", who, flags);
    Compacting how = {who, COMPACT_DECODE, (flags & KMPGPU_DECODE_ONLY_CHANGED) != 0};
    how.plus = (flags & KMPGPU_DECODE_PLUS) != 0;
    return recoded_call(dst, src, how, changed_out, d_changed, stats);
}

int kmpgpu_load_base64(kmpgpu_ctx *dst, kmpgpu_ctx *src, uint32_t min_run, uint32_t flags, uint64_t *changed_out, const void **d_changed,
                       kmpgpu_decode_stats *stats)
{
    const char *who = "kmpgpu_load_base64";
    if (d_changed) *d_changed = nullptr;
    if (stats) *stats = kmpgpu_decode_stats{};
    if (const int rc = pair_refused(dst, src, who)) return rc;
    if (min_run < 4u || min_run > 255u) return fail(KMPGPU_EINVAL, "%s: min_run %u is outside 4..255", who, min_run);
    if (flags & ~(KMPGPU_B64_URLSAFE | KMPGPU_B64_ONLY_CHANGED)) return fail(KMPGPU_EINVAL, "%s: unknown flag bits 0x%x", who, flags);
    Compacting how = {who, COMPACT_BASE64, (flags & KMPGPU_B64_ONLY_CHANGED) != 0};
    how.urlsafe = (flags & KMPGPU_B64_URLSAFE) != 0; how.min_run = min_run;
    return recoded_call(dst, src, how, changed_out, d_changed, stats);
}

/* kmpgpu_load_fields, kmpgpu_load_dns and kmpgpu_load_tls behind the checks of their own arguments */
static int field_buffer_call(kmpgpu_ctx *dst, kmpgpu_ctx *src, const Compacting &how, uint64_t *present_out, const void **d_present,
                             kmpgpu_fields_stats *stats)
{
    if (const int rc = pair_state_refused(dst, src, how.who, "field buffers")) return rc;
    uint64_t st[4] = {0, 0, 0, 0};
    const int rc = load_compacted(dst, src, how, present_out, d_present, st);
    if (!rc && stats) { stats->n_payloads = st[0]; stats->n_present = st[1]; stats->bytes_in = st[2]; stats->bytes_out = st[3]; }
    return rc;
}

int kmpgpu_load_fields(kmpgpu_ctx *dst, kmpgpu_ctx *src, int field, uint32_t flags, uint64_t *present_out, const void **d_present,
                       kmpgpu_fields_stats *stats)
{
    const char *who = "kmpgpu_load_fields";
    if (d_present) *d_present = nullptr;
    if (stats) *stats = kmpgpu_fields_stats{};
    if (const int rc = pair_refused(dst, src, who)) return rc;
    if (field < KMPGPU_FIELD_METHOD || field > KMPGPU_FIELD_BODY) return fail(KMPGPU_EINVAL, "%s: field %d is none of KMPGPU_FIELD_*", who, field);
    if (flags & ~KMPGPU_FIELDS_ONLY_PRESENT) return fail(KMPGPU_EINVAL, "%s: unknown flag bits 0x%x", who, flags);
    Compacting how = {who, COMPACT_FIELDS, (flags & KMPGPU_FIELDS_ONLY_PRESENT) != 0};
    how.field = field; how.sk = SpanKind{SPANS_HTTP, 0u};
    return field_buffer_call(dst, src, how, present_out, d_present, stats);
}

int kmpgpu_load_dns(kmpgpu_ctx *dst, kmpgpu_ctx *src, int field, uint32_t flags, uint64_t *present_out, const void **d_present,
                    kmpgpu_fields_stats *stats)
{
    const char *who = "kmpgpu_load_dns";
    if (d_present) *d_present = nullptr;
    if (stats) *stats = kmpgpu_fields_stats{};
    if (const int rc = pair_refused(dst, src, who)) return rc;
    if (field != KMPGPU_DNS_QNAME) return fail(KMPGPU_EINVAL, "%s: field %d is not KMPGPU_DNS_QNAME", who, field);
    if (flags & ~(KMPGPU_DNS_ONLY_PRESENT | KMPGPU_DNS_TCP_PREFIX)) return fail(KMPGPU_EINVAL, "%s: unknown flag bits 0x%x", who, flags);
    Compacting how = {who, COMPACT_DNS, (flags & KMPGPU_DNS_ONLY_PRESENT) != 0};
    how.field = field; how.sk = SpanKind{SPANS_DNS, flags & KMPGPU_DNS_TCP_PREFIX};
    return field_buffer_call(dst, src, how, present_out, d_present, stats);
}

int kmpgpu_load_tls(kmpgpu_ctx *dst, kmpgpu_ctx *src, int field, uint32_t flags, uint64_t *present_out, const void **d_present,
                    kmpgpu_fields_stats *stats)
{
    const char *who = "kmpgpu_load_tls";
    if (d_present) *d_present = nullptr;
    if (stats) *stats = kmpgpu_fields_stats{};
    if (const int rc = pair_refused(dst, src, who)) return rc;
    if (field != KMPGPU_TLS_SNI && field != KMPGPU_TLS_ALPN) return fail(KMPGPU_EINVAL, "%s: field %d is neither KMPGPU_TLS_SNI nor KMPGPU_TLS_ALPN", who, field);
    if (flags & ~KMPGPU_TLS_ONLY_PRESENT) return fail(KMPGPU_EINVAL, "%s: unknown flag bits 0x%x", who, flags);
    Compacting how = {who, COMPACT_TLS, (flags & KMPGPU_TLS_ONLY_PRESENT) != 0};
    how.field = field; how.sk = SpanKind{SPANS_TLS, 0u};
    return field_buffer_call(dst, src, how, present_out, d_present, stats);
}

int kmpgpu_load_seams(kmpgpu_ctx *dst, kmpgpu_ctx *src, uint32_t reach, uint64_t *n_seams)
{
    const char *who = "kmpgpu_load_seams";
    if (n_seams) *n_seams = 0;
    if (const int rc = pair_refused(dst, src, who)) return rc;
    if (reach < 1u || reach > KMPGPU_MAX_PATTERN_LEN - 1u)
        return fail(KMPGPU_EINVAL, "%s: reach %u is not in 1..%u", who, reach, KMPGPU_MAX_PATTERN_LEN - 1u);
    if (const int rc = pair_state_refused(dst, src, who, "seams")) return rc;
    if (!src->flows_valid) return fail(KMPGPU_ESTATE, "%s: no flows (no kmpgpu_flows_build since the arena or its metadata were set)", who);
    if (const int rc = derived_begin(dst, src)) return rc;
    kmpgpu_ctx *c = dst;
    const uint64_t n = src->n_pkts;
    /* from here on dst's earlier arena is gone, whatever happens */
    release_arena(c, /* keep_buffers = */ true);
    auto listed = [&](uint64_t ns) {
        c->n_seams = ns; c->seam_src = src->id; c->seam_gen = src->flows_gen; c->seams_valid = true;
        if (n_seams) *n_seams = ns;
        return KMPGPU_OK;
    };
    if (n == 0) return listed(0);

    /* the scratch of kmpgpu_load_frames (fr_ws the scan, fr_src the gather's records) and the sort's own buffer */
    if (const int rc = flow_sort_scratch(c, src, who, (uint64_t)kmp_extract_ws_bytes(n))) return rc;
    if (const int rc = sort_by_flow(c, src)) return rc;
    HIP_TRY(profiled(c, [&] { return kmp_launch_seam_phase1(src->d_len, n, reach, c->d_seam_sort, c->fr_ws, c->fr_tot, c->stream); }));
    unsigned long long tot[2] = {0, 0};
    if (const int rc = read_totals(c, tot)) return rc;
    const uint64_t ns = tot[1];
    if (ns == 0) {
        if (const int rc = derived_finish(c, 5, /* record = */ true)) return rc;
        return listed(0);
    }
    if (const int rc = take_arena(c, who, tot[0], ns, "seams")) return rc;
    hipError_t e = grow_buffer(&c->fr_src, &c->fr_src_cap, 4 * ns, EIGHTH);  /* 32 bytes per seam */
    if (e == hipSuccess) e = grow_buffer(&c->d_meta, &c->meta_cap, ns, EIGHTH);
    if (e == hipSuccess) e = grow_buffer(&c->d_seams, &c->seams_cap, ns, EIGHTH);
    if (e == hipSuccess) e = grow_buffer(&c->d_seam_flow, &c->seam_flow_cap, ns, EIGHTH);
    if (e != hipSuccess) return alloc_fail(e, "%s: the records of %llu seams could not be allocated", who, (unsigned long long)ns);
    HIP_TRY(profiled(c, [&] {
        return kmp_launch_seam_index(src->d_off, src->d_len, src->d_meta, src->d_flow_of, n, reach, c->fr_ws, c->owned_off, c->owned_len, c->d_seams,
                                     c->d_seam_flow, c->d_meta, c->fr_src, c->stream);
    }));
    HIP_TRY(profiled(c, [&] {
        return kmp_launch_seam_gather(src->d_arena, c->owned_off, c->fr_src, ns, tot[0], c->owned_arena, c->nontemporal != 0, c->stream);
    }));
    HIP_TRY(hipEventRecord(c->ev[3], c->stream));
    if (const int rc = install_owned(c, who, tot[0], ns)) return rc;
    if (const int rc = derived_finish(c, 7, /* record = */ false)) return rc;
    c->has_meta = true;
    return listed(ns);
}

int kmpgpu_seams_read(kmpgpu_ctx *c, kmpgpu_seam *out, uint64_t first, uint64_t n)
{
    static_assert(sizeof(kmpgpu_seam) == 24, "kmpgpu_seam is the 24-byte record of kmpgpu.h");
    const char *who = "kmpgpu_seams_read";
    if (!c) return fail(KMPGPU_EINVAL, "%s: ctx is NULL", who);
    return read_range(c, who, c->seams_valid, "no seams (no kmpgpu_load_seams since the arena was set)", out, c->d_seams, sizeof(kmpgpu_seam), first, n,
                      c->n_seams);
}

/* kmpgpu_load_streams and kmpgpu_load_streams_ordered behind their checks: the streams in capture order, or, ordered, with the second
 * sort, its scans, and the records, index and gather that follow the sequence numbers. */
static int load_streams_call(kmpgpu_ctx *dst, kmpgpu_ctx *src, const char *who, uint32_t depth, bool ordered, const uint32_t *seq, bool on_device,
                             uint64_t *n_streams)
{
    if (const int rc = derived_begin(dst, src)) return rc;
    kmpgpu_ctx *c = dst;
    const uint64_t n = src->n_pkts;
    /* from here on dst's earlier arena is gone, whatever happens */
    release_arena(c, /* keep_buffers = */ true);
    if (n == 0) { c->streams_valid = true; c->stream_order_valid = ordered; return KMPGPU_OK; }       /* (no stream, no map entry) */

    /* the scratch of kmpgpu_load_frames (fr_ws the scans, fr_src the gather's pieces), the sort buffer of kmpgpu_load_seams, and for the
     * sequence order the second sort's and its scans' workspace and the copy of a host seq: all of it sized and taken before the seq is
     * uploaded, so that no return for a size or for memory leaves a copy out of the caller's seq under way */
    const uint64_t seq_bytes = ordered ? kmp_stream_seq_ws_bytes(n, src->n_flows) : 0;
    if (ordered && !seq_bytes) return fail(KMPGPU_EHIP, "%s: the second sort of %llu payloads could not be sized", who, (unsigned long long)n);
    if (const int rc = flow_sort_scratch(c, src, who, (uint64_t)kmp_stream_ws_bytes(n))) return rc;
    hipError_t e = grow_buffer(&c->fr_src, &c->fr_src_cap, 3 * n, EIGHTH);                         /* 24 bytes per source payload */
    if (e == hipSuccess) e = grow_buffer(&c->d_stream_map, &c->stream_map_cap, n, EIGHTH);
    if (e == hipSuccess && ordered) e = grow_buffer(&c->d_stream_seq_ws, &c->stream_seq_ws_cap, seq_bytes, EIGHTH);
    if (e == hipSuccess && ordered) e = grow_buffer(&c->d_stream_segs, &c->stream_segs_cap, n, EIGHTH);
    if (e == hipSuccess && ordered && !on_device) e = grow_buffer(&c->d_stream_seq, &c->stream_seq_cap, n, EIGHTH);
    if (e != hipSuccess) return alloc_fail(e, "%s: the scans' buffers (%llu payloads) could not be allocated", who, (unsigned long long)n);
    const uint32_t *d_seq = seq;
    if (ordered && !on_device) {
        HIP_TRY(upload_split(c->d_stream_seq, reinterpret_cast<const uint8_t *>(seq), n * sizeof(uint32_t), c->stream));
        d_seq = c->d_stream_seq;
    }
    if (const int rc = sort_by_flow(c, src)) return rc;
    HIP_TRY(profiled(c, [&] { return kmp_launch_stream_phase1(src->d_len, n, c->d_seam_sort, c->fr_ws, c->fr_tot, c->stream); }));
    unsigned long long tot[2] = {0, 0};
    if (const int rc = read_totals(c, tot)) return rc;
    const uint64_t total = tot[0], ns = tot[1];                              /* bytes of all members; streams, at least one */
    e = grow_buffer(&c->d_streams, &c->streams_cap, ns, EIGHTH);
    if (e == hipSuccess && ordered) e = grow_buffer(&c->d_stream_orders, &c->stream_orders_cap, ns, EIGHTH);
    if (e == hipSuccess) e = grow_buffer(&c->d_meta, &c->meta_cap, ns, EIGHTH);
    if (e != hipSuccess) return alloc_fail(e, "%s: the records of %llu streams could not be allocated", who, (unsigned long long)ns);
    if (ordered) {
        HIP_TRY(profiled(c, [&] {
            return kmp_launch_stream_seq_order(src->d_meta, d_seq, n, ns, src->n_flows, c->d_seam_sort, c->fr_ws, c->d_stream_seq_ws,
                                               (size_t)c->stream_seq_ws_cap, c->stream);
        }));
        HIP_TRY(profiled(c, [&] { return kmp_launch_stream_seq_scans(src->d_len, n, c->d_seam_sort, c->fr_ws, c->d_stream_seq_ws, c->stream); }));
        HIP_TRY(profiled(c, [&] {
            return kmp_launch_stream_seq_records(src->d_meta, d_seq, n, total, ns, depth, c->d_seam_sort, c->fr_ws, c->d_stream_seq_ws, c->d_streams,
                                                 c->d_stream_orders, c->d_meta, c->fr_tot, c->stream);
        }));
    } else {
        HIP_TRY(profiled(c, [&] {
            return kmp_launch_stream_records(src->d_meta, n, total, ns, depth, c->d_seam_sort, c->fr_ws, c->d_streams, c->d_meta, c->fr_tot, c->stream);
        }));
    }
    /* the second read: the arena's size follows from the cut lengths, which follow from the first read's n_streams */
    if (const int rc = read_totals(c, tot)) return rc;
    if (const int rc = take_arena(c, who, tot[0], ns, "streams")) return rc;
    HIP_TRY(profiled(c, [&] {
        if (ordered)
            return kmp_launch_stream_seq_index(src->d_off, src->d_len, n, ns, c->d_seam_sort, c->fr_ws, c->d_stream_seq_ws, c->owned_off, c->owned_len,
                                               c->d_stream_map, c->d_stream_segs, c->fr_src, c->stream);
        return kmp_launch_stream_index(src->d_off, src->d_len, n, total, ns, c->d_seam_sort, c->fr_ws, c->owned_off, c->owned_len, c->d_stream_map,
                                       c->fr_src, c->stream);
    }));
    HIP_TRY(profiled(c, [&] {
        if (ordered) return kmp_launch_stream_seq_gather(src->d_arena, c->fr_src, n, tot[0], c->owned_arena, c->nontemporal != 0, c->stream);
        return kmp_launch_stream_gather(src->d_arena, c->fr_src, n, tot[0], c->owned_arena, c->nontemporal != 0, c->stream);
    }));
    HIP_TRY(hipEventRecord(c->ev[3], c->stream));
    if (const int rc = install_owned(c, who, tot[0], ns)) return rc;
    if (const int rc = derived_finish(c, ordered ? 16 : 10, /* record = */ false)) return rc;
    c->has_meta = true;
    c->n_streams = ns; c->n_stream_map = n; c->streams_valid = true; c->stream_order_valid = ordered;
    if (n_streams) *n_streams = ns;
    return KMPGPU_OK;
}

int kmpgpu_load_streams(kmpgpu_ctx *dst, kmpgpu_ctx *src, uint32_t depth, uint64_t *n_streams)
{
    const char *who = "kmpgpu_load_streams";
    if (n_streams) *n_streams = 0;
    if (const int rc = pair_refused(dst, src, who)) return rc;
    if (depth < 1u || depth > KMPGPU_STREAM_DEPTH_MAX)
        return fail(KMPGPU_EINVAL, "%s: depth %u is not in 1..%u", who, depth, KMPGPU_STREAM_DEPTH_MAX);
    if (const int rc = pair_state_refused(dst, src, who, "streams")) return rc;
    if (!src->flows_valid) return fail(KMPGPU_ESTATE, "%s: no flows (no kmpgpu_flows_build since the arena or its metadata were set)", who);
    return load_streams_call(dst, src, who, depth, /* ordered = */ false, nullptr, false, n_streams);
}

/* what the four reads of the stream state share */
static int streams_read_range(kmpgpu_ctx *c, const char *who, void *out, const void *list, size_t size, uint64_t first, uint64_t n, uint64_t total)
{
    return read_range(c, who, c->streams_valid, "no streams (no kmpgpu_load_streams since the arena was set)", out, list, size, first, n, total);
}

int kmpgpu_streams_read(kmpgpu_ctx *c, kmpgpu_stream *out, uint64_t first, uint64_t n)
{
    static_assert(sizeof(kmpgpu_stream) == 48, "kmpgpu_stream is the 48-byte record of kmpgpu.h");
    if (!c) return fail(KMPGPU_EINVAL, "kmpgpu_streams_read: ctx is NULL");
    return streams_read_range(c, "kmpgpu_streams_read", out, c->d_streams, sizeof(kmpgpu_stream), first, n, c->n_streams);
}

int kmpgpu_stream_map_read(kmpgpu_ctx *c, kmpgpu_stream_pos *out, uint64_t first, uint64_t n)
{
    static_assert(sizeof(kmpgpu_stream_pos) == 16, "kmpgpu_stream_pos is the 16-byte record of kmpgpu.h");
    if (!c) return fail(KMPGPU_EINVAL, "kmpgpu_stream_map_read: ctx is NULL");
    return streams_read_range(c, "kmpgpu_stream_map_read", out, c->d_stream_map, sizeof(kmpgpu_stream_pos), first, n, c->n_stream_map);
}

int kmpgpu_load_streams_ordered(kmpgpu_ctx *dst, kmpgpu_ctx *src, uint32_t depth, const uint32_t *seq, int on_device, uint64_t *n_streams)
{
    const char *who = "kmpgpu_load_streams_ordered";
    if (n_streams) *n_streams = 0;
    if (const int rc = pair_refused(dst, src, who)) return rc;
    if (depth < 1u || depth > KMPGPU_STREAM_DEPTH_MAX)
        return fail(KMPGPU_EINVAL, "%s: depth %u is not in 1..%u", who, depth, KMPGPU_STREAM_DEPTH_MAX);
    if (on_device != 0 && on_device != 1) return fail(KMPGPU_EINVAL, "%s: on_device %d is neither 0 nor 1", who, on_device);
    if (const int rc = pair_state_refused(dst, src, who, "streams")) return rc;
    const uint64_t n = src->n_pkts;
    if (n > (1ull << 30)) return fail(KMPGPU_EINVAL, "%s: %llu payloads are more than 2^30 (the composite sort keys)", who, (unsigned long long)n);
    if (!seq && n > 0) return fail(KMPGPU_EINVAL, "%s: seq is NULL", who);
    if (n > 0 && !src->has_meta) return fail(KMPGPU_ESTATE, "%s: src has no metadata (which stream is TCP is read from it)", who);
    if (!src->flows_valid) return fail(KMPGPU_ESTATE, "%s: no flows (no kmpgpu_flows_build since the arena or its metadata were set)", who);
    return load_streams_call(dst, src, who, depth, /* ordered = */ true, seq, on_device != 0, n_streams);
}

/* the two reads that exist for streams in sequence order only */
static int stream_order_read(kmpgpu_ctx *c, const char *who, void *out, const void *list, size_t size, uint64_t first, uint64_t n, uint64_t total)
{
    if (c->streams_valid && !c->stream_order_valid) return fail(KMPGPU_ESTATE, "%s: no sequence order (the streams were built by kmpgpu_load_streams)", who);
    return streams_read_range(c, who, out, list, size, first, n, total);
}

int kmpgpu_stream_segs_read(kmpgpu_ctx *c, kmpgpu_stream_seg *out, uint64_t first, uint64_t n)
{
    static_assert(sizeof(kmpgpu_stream_seg) == 16, "kmpgpu_stream_seg is the 16-byte record of kmpgpu.h");
    if (!c) return fail(KMPGPU_EINVAL, "kmpgpu_stream_segs_read: ctx is NULL");
    return stream_order_read(c, "kmpgpu_stream_segs_read", out, c->d_stream_segs, sizeof(kmpgpu_stream_seg), first, n, c->n_stream_map);
}

int kmpgpu_stream_orders_read(kmpgpu_ctx *c, kmpgpu_stream_order *out, uint64_t first, uint64_t n)
{
    static_assert(sizeof(kmpgpu_stream_order) == 32, "kmpgpu_stream_order is the 32-byte record of kmpgpu.h");
    if (!c) return fail(KMPGPU_EINVAL, "kmpgpu_stream_orders_read: ctx is NULL");
    return stream_order_read(c, "kmpgpu_stream_orders_read", out, c->d_stream_orders, sizeof(kmpgpu_stream_order), first, n, c->n_streams);
}

int kmpgpu_scan_enqueue(kmpgpu_ctx *c, void *d_counts_out)
{
    if (!c) return fail(KMPGPU_EINVAL, "kmpgpu_scan_enqueue: ctx is NULL");
    if ((uintptr_t)d_counts_out & 7u) return fail(KMPGPU_EINVAL, "kmpgpu_scan_enqueue: d_counts_out is not 8-byte aligned");
    HIP_TRY(hipSetDevice(c->device));
    return enqueue_pass(c, nullptr, (unsigned long long *)d_counts_out, c->accumulate != 0);
}

void *kmpgpu_counts_device(kmpgpu_ctx *c) { return c ? (void *)c->d_counts : nullptr; }

int kmpgpu_counts_reset(kmpgpu_ctx *c)
{
    if (!c) return fail(KMPGPU_EINVAL, "kmpgpu_counts_reset: ctx is NULL");
    if (!c->d_counts) return fail(KMPGPU_ESTATE, "kmpgpu_counts_reset: no patterns set");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemsetAsync(c->d_counts, 0, sizeof(unsigned long long) * (c->n_pat ? c->n_pat : 1), c->stream));
    return KMPGPU_OK;
}

int kmpgpu_counts_add(kmpgpu_ctx *dst, kmpgpu_ctx *src)
{
    if (!dst || !src || dst == src) return fail(KMPGPU_EINVAL, "kmpgpu_counts_add: bad arguments");
    if (dst->device != src->device) return fail(KMPGPU_EINVAL, "kmpgpu_counts_add: the contexts sit on devices %d and %d (sum across devices with kmpgpu_comm_allreduce_counts)", dst->device, src->device);
    if (!dst->d_counts || !src->d_counts || dst->n_pat != src->n_pat) return fail(KMPGPU_ESTATE, "kmpgpu_counts_add: the contexts do not hold the same patterns");
    HIP_TRY(hipSetDevice(dst->device));
    HIP_TRY(hipStreamSynchronize(src->stream));                 /* src's passes have landed in its counters */
    HIP_TRY(kmp_launch_add_counts(dst->d_counts, src->d_counts, dst->n_pat, dst->stream));
    return KMPGPU_OK;
}

int kmpgpu_last_timing(kmpgpu_ctx *c, kmpgpu_timing *t)
{
    if (!c || !t) return fail(KMPGPU_EINVAL, "kmpgpu_last_timing: NULL argument");
    *t = c->last;
    return KMPGPU_OK;
}

int kmpgpu_counts_read(kmpgpu_ctx *c, uint64_t *counts_out)
{
    if (!c || (!counts_out && c->n_pat)) return fail(KMPGPU_EINVAL, "kmpgpu_counts_read: NULL argument");
    if (!c->d_counts) return fail(KMPGPU_ESTATE, "kmpgpu_counts_read: no patterns set");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(c->h_counts, c->d_counts, sizeof(uint64_t) * c->n_pat, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->n_pat) memcpy(counts_out, c->h_counts, sizeof(uint64_t) * c->n_pat);
    return KMPGPU_OK;
}

int kmpgpu_sync(kmpgpu_ctx *c)
{
    if (!c) return fail(KMPGPU_EINVAL, "kmpgpu_sync: ctx is NULL");
    HIP_TRY(hipStreamSynchronize(c->stream));
    return KMPGPU_OK;
}

int kmpgpu_scan(kmpgpu_ctx *c, uint64_t *counts_out, kmpgpu_timing *t)
{
    if (!c) return fail(KMPGPU_EINVAL, "kmpgpu_scan: ctx is NULL");
    if (!counts_out && c->n_pat) return fail(KMPGPU_EINVAL, "kmpgpu_scan: counts_out is NULL");
    HIP_TRY(hipSetDevice(c->device));
    uint32_t launches = 0;
    HIP_TRY(hipEventRecord(c->ev[0], c->stream));
    int rc = enqueue_pass(c, &launches, nullptr, c->accumulate != 0);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(c->ev[1], c->stream));
    HIP_TRY(hipMemcpyAsync(c->h_counts, c->d_counts, sizeof(uint64_t) * c->n_pat, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipEventRecord(c->ev[2], c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    float k_ms = 0, d_ms = 0;
    HIP_TRY(hipEventElapsedTime(&k_ms, c->ev[0], c->ev[1]));
    HIP_TRY(hipEventElapsedTime(&d_ms, c->ev[1], c->ev[2]));
    memcpy(counts_out, c->h_counts, sizeof(uint64_t) * c->n_pat);
    c->last.kernel_ms = k_ms; c->last.d2h_ms = d_ms; c->last.launches = launches;
    c->last.grid_blocks = c->n_pkts ? grid_blocks(c, primary_set(c)) : 0;
    if (t) *t = c->last;
    return KMPGPU_OK;
}

int kmpgpu_profile_begin(kmpgpu_ctx *c, uint32_t max_launches)
{
    if (!c) return fail(KMPGPU_EINVAL, "kmpgpu_profile_begin: ctx is NULL");
    HIP_TRY(hipSetDevice(c->device));
    while (c->prof_ev.size() < 2 * (size_t)max_launches) {
        hipEvent_t e;
        HIP_TRY(hipEventCreate(&e));
        c->prof_ev.push_back(e);
    }
    c->prof_cap = max_launches; c->prof_n = 0; c->profiling = true;
    return KMPGPU_OK;
}

int kmpgpu_profile_end(kmpgpu_ctx *c, float *ms_out, uint32_t *n)
{
    if (!c || !n) return fail(KMPGPU_EINVAL, "kmpgpu_profile_end: NULL argument");
    c->profiling = false;
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (uint32_t i = 0; i < c->prof_n; i++) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, c->prof_ev[2 * i], c->prof_ev[2 * i + 1]));
        if (ms_out) ms_out[i] = ms;
    }
    *n = c->prof_n;
    c->prof_n = 0;
    return KMPGPU_OK;
}

int kmpgpu_scan_offsets(kmpgpu_ctx *c, kmpgpu_match *out, uint64_t cap, uint64_t *n_found, uint64_t *counts_out)
{
    if (!c || !n_found) return fail(KMPGPU_EINVAL, "kmpgpu_scan_offsets: NULL argument");
    if (cap && !out) return fail(KMPGPU_EINVAL, "kmpgpu_scan_offsets: out is NULL");
    if (c->mode != 0 || c->kernel_sel == 1) return fail(KMPGPU_EINVAL, "kmpgpu_scan_offsets runs on the streaming kernels only (mode 0, kernel 0, 2 or 3)");
    static_assert(sizeof(kmpgpu_match) == 16, "kmpgpu_match is a 16-byte record");
    HIP_TRY(hipSetDevice(c->device));
    *n_found = 0;
    if (!c->packed && c->n_pkts) {
        /* an arena kept in place (KMPGPU_OPT_REPACK = 0) whose slots are not back to back: the offsets come from the
         * streaming kernels, so it is packed now, once (the context scans its packed copy from here on) */
        HIP_TRY(hipStreamSynchronize(c->stream));
        const int rr = repack_arena(c);
        if (rr) return rr;
    }
    void *d_out = nullptr;
    unsigned long long *d_cnt = nullptr;             /* [0] matches found; [1 ..] this pass's counts */
    const size_t np = c->n_pat ? c->n_pat : 1;
    HIP_TRY(hipMalloc(&d_out, (cap ? cap : 1) * sizeof(kmpgpu_match)));
    hipError_t e = hipMalloc(&d_cnt, (1 + np) * sizeof(unsigned long long));
    int rc = KMPGPU_OK;
    unsigned long long found = 0;
    if (e != hipSuccess) rc = fail(KMPGPU_EHIP, "hipMalloc failed: %s", hipGetErrorString(e));
    if (!rc && (e = hipMemsetAsync(d_cnt, 0, (1 + np) * sizeof(unsigned long long), c->stream)) != hipSuccess)
        rc = fail(KMPGPU_EHIP, "hipMemsetAsync failed: %s", hipGetErrorString(e));
    if (!rc) {
        /* The pass writes its counts to a buffer of its own and never accumulates: the context's counters (a running
         * total under KMPGPU_OPT_ACCUMULATE, or the result of a count reduce) are left as they are. */
        EmitTarget t;
        t.out = d_out; t.counter = d_cnt; t.cap = cap;
        rc = enqueue_pass(c, nullptr, d_cnt + 1, /* accumulate = */ false, &t);
    }
    if (!rc && (e = hipMemcpyAsync(&found, d_cnt, sizeof found, hipMemcpyDeviceToHost, c->stream)) != hipSuccess)
        rc = fail(KMPGPU_EHIP, "hipMemcpyAsync failed: %s", hipGetErrorString(e));
    if (!rc && c->n_pat && counts_out &&
        (e = hipMemcpyAsync(c->h_counts, d_cnt + 1, sizeof(uint64_t) * c->n_pat, hipMemcpyDeviceToHost, c->stream)) != hipSuccess)
        rc = fail(KMPGPU_EHIP, "hipMemcpyAsync failed: %s", hipGetErrorString(e));
    if (!rc && (e = hipStreamSynchronize(c->stream)) != hipSuccess) rc = fail(KMPGPU_EHIP, "hipStreamSynchronize failed: %s", hipGetErrorString(e));
    if (!rc) {
        const unsigned long long n = found < cap ? found : cap;
        if (n && (e = hipMemcpy(out, d_out, n * sizeof(kmpgpu_match), hipMemcpyDeviceToHost)) != hipSuccess)
            rc = fail(KMPGPU_EHIP, "hipMemcpy failed: %s", hipGetErrorString(e));
        if (counts_out && c->n_pat) memcpy(counts_out, c->h_counts, sizeof(uint64_t) * c->n_pat);
        *n_found = found;
    }
    (void)hipFree(d_out);
    if (d_cnt) (void)hipFree(d_cnt);
    return rc;
}

namespace {

/* The marking pass every row family starts with: preconditions, the arena packed where it was kept in place, the context's matrix buffer
 * grown and zeroed, and the scan launches that mark it.  Leaves c->ev[0] recorded in front of the zeroing.
 * empty: no payloads, nothing was enqueued. */
struct MarkPass {
    bool empty = false;
    uint64_t W = 0, stride = 0, mat = 0;          /* words per row as the caller sees them / on the device (even); words of the matrix */
    unsigned long long *d_mat = nullptr, *d_cnt = nullptr;       /* [n_pat + n_rel + n_chains + n_hdr + n_bt + n_rx + n_links][stride]; the scan's counts [n_pat] */
    uint32_t launches = 0;
};

int marking_pass(kmpgpu_ctx *c, const char *who, MarkPass *p)
{
    if (c->mode != 0 || c->kernel_sel == 1) return fail(KMPGPU_EINVAL, "%s runs on the streaming kernels only (mode 0, kernel 0, 2 or 3)", who);
    if (!c->d_patterns || c->n_pat == 0) return fail(KMPGPU_ESTATE, "%s: no patterns set", who);
    if (!c->d_off && c->n_pkts) return fail(KMPGPU_ESTATE, "%s: no arena loaded", who);
    HIP_TRY(hipSetDevice(c->device));
    *p = MarkPass{};
    p->W = (c->n_pkts + 63u) / 64u;
    const size_t np = c->n_pat;
    if (c->n_pkts == 0) { p->empty = true; return KMPGPU_OK; }
    /* rows of an even number of words: the reduce and the rules kernel read 16 bytes per lane */
    const uint64_t stride = (p->W + 1u) & ~1ull;
    if (stride > 0xFFFFFFFEull) return fail(KMPGPU_EINVAL, "%s: too many payloads for the hit matrix", who);
    if (!c->packed) {
        /* an arena kept in place (KMPGPU_OPT_REPACK = 0) whose slots are not back to back: packed now, once (kmpgpu_scan_offsets) */
        HIP_TRY(hipStreamSynchronize(c->stream));
        const int rr = repack_arena(c);
        if (rr) return rr;
    }
    /* one device buffer, grown like the others: [marks (n_pat + n_rel + n_chains + n_hdr + n_bt + n_rx + n_links) x stride][pkt_counts n_pat]
     * [any stride][counts n_pat][rel_pkt_counts n_rel][chain_pkt_counts n_chains][hdr_pkt_counts n_hdr][bt_pkt_counts n_bt][rx_pkt_counts n_rx]
     * [link_pkt_counts n_links]; the scan kernels mark rows 0 .. n_pat - 1, the relation kernel, the chain kernel, the header kernel, the
     * byte-test kernels and the regex kernel write the rows behind them, the link rows are copied in behind those (family_rows) */
    const uint64_t mat = ((uint64_t)np + c->n_rel + c->n_chains + c->n_hdr + c->n_bt + c->n_rx + c->n_links) * stride;
    const uint64_t words = mat + np + stride + np + c->n_rel + c->n_chains + c->n_hdr + c->n_bt + c->n_rx + c->n_links;
    hipError_t e = grow_buffer(&c->d_marks, &c->marks_cap, words, EIGHTH);
    if (e != hipSuccess) return alloc_fail(e, "%s: the hit matrix (%llu bytes) could not be allocated", who, (unsigned long long)(words * 8u));
    p->stride = stride; p->mat = mat;
    p->d_mat = c->d_marks; p->d_cnt = p->d_mat + mat + np + stride;
    HIP_TRY(hipEventRecord(c->ev[0], c->stream));
    /* zeroed before every pass: the bits of an earlier (larger) arena must not leak into this one */
    HIP_TRY(hipMemsetAsync(p->d_mat, 0, (size_t)words * sizeof(unsigned long long), c->stream));
    /* the pass writes its counts to a buffer of its own and never accumulates: the context's counters stay as they are */
    EmitTarget tg;
    tg.out = nullptr; tg.counter = nullptr; tg.cap = 0;
    tg.marks = p->d_mat; tg.mark_stride = (uint32_t)stride;
    return enqueue_pass(c, &p->launches, p->d_cnt, /* accumulate = */ false, &tg);
}

/* rows of W words from a device matrix whose rows are `stride` words apart */
hipError_t download_rows(kmpgpu_ctx *c, uint64_t *dst, const unsigned long long *src, uint64_t W, uint64_t stride, uint64_t rows)
{
    if (stride == W) return hipMemcpyAsync(dst, src, (size_t)(rows * W) * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream);
    return hipMemcpy2DAsync(dst, W * sizeof(uint64_t), src, stride * sizeof(uint64_t), W * sizeof(uint64_t), rows, hipMemcpyDeviceToHost, c->stream);
}

/* the header predicates' rows: a family of kmpgpu_scan_headers and of the rules' terms, none of kmpgpu_scan_alerts (kmpgpu.h) */
constexpr int FAMILY_HEADERS = KMPGPU_ALERT_CHAINS + 1;
/* ... and the byte tests': a family of kmpgpu_scan_bytetests and of the rules' terms */
constexpr int FAMILY_BYTETESTS = KMPGPU_ALERT_CHAINS + 2;
/* ... and the expressions': a family of kmpgpu_scan_regexes and of the rules' terms */
constexpr int FAMILY_REGEXES = KMPGPU_ALERT_CHAINS + 3;
/* ... and the links': a family of kmpgpu_scan_links and of the rules' terms */
constexpr int FAMILY_LINKS = KMPGPU_ALERT_CHAINS + 4;

/* A row family (KMPGPU_ALERT_*, FAMILY_HEADERS, FAMILY_BYTETESTS, FAMILY_REGEXES, FAMILY_LINKS): patterns, rules, relations, chains, header predicates, byte tests, expressions or links.  Where its results lie on the device once its kernels are
 * enqueued behind a marking pass (enqueue_family). */
struct FamilyRows {
    unsigned long long *d_rows = nullptr, *d_pc = nullptr, *d_any = nullptr;     /* [n_rows][stride], payloads per row [n_rows], [stride] */
    uint64_t n_rows = 0;
    uint32_t launches = 0;                        /* added to the marking pass's */
};

uint64_t family_n_rows(const kmpgpu_ctx *c, int family)
{
    return family == KMPGPU_ALERT_PATTERNS ? c->n_pat : family == KMPGPU_ALERT_RULES ? c->n_rules : family == KMPGPU_ALERT_RELATIONS ? c->n_rel
         : family == KMPGPU_ALERT_CHAINS ? c->n_chains : family == FAMILY_HEADERS ? c->n_hdr : family == FAMILY_BYTETESTS ? c->n_bt : family == FAMILY_REGEXES ? c->n_rx : c->n_links;
}

/* The one place that knows where the families live: the patterns, relations, chains, header predicates, byte tests, expressions and links in the marks buffer as marking_pass lays it out
 * (they share its any[]; one family's kernel writes it per pass), the rules in the context's rule buffer [rule rows n_rules x stride]
 * [rule_pkt_counts n_rules][any stride]. */
void family_rows(const kmpgpu_ctx *c, const MarkPass &p, int family, FamilyRows *f)
{
    *f = FamilyRows{};
    f->n_rows = family_n_rows(c, family);
    if (family == KMPGPU_ALERT_RULES) {
        f->d_rows = c->d_rule_out; f->d_pc = f->d_rows + f->n_rows * p.stride; f->d_any = f->d_pc + f->n_rows;
        return;
    }
    const uint64_t np = c->n_pat, first = family == KMPGPU_ALERT_PATTERNS ? 0 : family == KMPGPU_ALERT_RELATIONS ? np
                                        : family == KMPGPU_ALERT_CHAINS ? np + c->n_rel : family == FAMILY_HEADERS ? np + c->n_rel + c->n_chains
                                        : family == FAMILY_BYTETESTS ? np + c->n_rel + c->n_chains + c->n_hdr
                                        : family == FAMILY_REGEXES ? np + c->n_rel + c->n_chains + c->n_hdr + c->n_bt
                                        : np + c->n_rel + c->n_chains + c->n_hdr + c->n_bt + c->n_rx;
    f->d_rows = p.d_mat + first * p.stride;
    f->d_pc = family == KMPGPU_ALERT_PATTERNS ? p.d_mat + p.mat : p.d_cnt + first;      /* (the counts of the rows behind the patterns': behind the scan's counts) */
    f->d_any = p.d_mat + p.mat + np;
}

/* The relation kernel or the chain kernel behind a marking pass: the family's rows of the matrix, their popcounts and their OR into any[]
 * (all zeroed by the pass; kmpgpu_scan_rules has no other use for that any[]).  One launch, recorded by a running profile. */
int enqueue_pairing(kmpgpu_ctx *c, const MarkPass &p, int family)
{
    const bool rel = family == KMPGPU_ALERT_RELATIONS;
    FamilyRows f;
    family_rows(c, p, family, &f);
    HIP_TRY(profiled(c, [&] {
        return (rel ? kmp_launch_relations : kmp_launch_chains)(p.d_mat, p.stride, c->n_pkts, rel ? c->d_relations : c->d_chains, (uint32_t)f.n_rows,
                                                                c->d_patterns, c->d_arena, c->d_fold, c->d_off, c->d_len, c->d_windows,
                                                                c->whole_payload != 0, (uint32_t)c->cu_count * 8u, f.d_rows, f.d_pc, f.d_any,
                                                                c->stream);
    }));
    return KMPGPU_OK;
}

/* The header kernel behind a marking pass, in the same way: the predicates' rows from the metadata and the index's lengths alone. */
int enqueue_headers(kmpgpu_ctx *c, const MarkPass &p)
{
    FamilyRows f;
    family_rows(c, p, FAMILY_HEADERS, &f);
    HIP_TRY(profiled(c, [&] {
        return kmp_launch_headers(c->d_meta, c->d_len, c->n_pkts, p.stride, c->d_headers, (uint32_t)f.n_rows, f.d_rows, f.d_pc, f.d_any, c->stream);
    }));
    return KMPGPU_OK;
}

/* The byte-test kernels behind a marking pass, in the same way: one for the absolute tests, one for the relative ones, each only where there
 * are some.  *launches: how many that were. */
int enqueue_bytetests(kmpgpu_ctx *c, const MarkPass &p, uint32_t *launches)
{
    FamilyRows f;
    family_rows(c, p, FAMILY_BYTETESTS, &f);
    const uint32_t *rel_idx = reinterpret_cast<const uint32_t *>(c->d_bytetests) + (size_t)c->n_bt * 8u;
    for (int relative = 0; relative < 2; relative++) {
        if (relative ? c->n_bt_rel == 0 : c->n_bt_rel == c->n_bt) continue;
        HIP_TRY(profiled(c, [&] {
            return kmp_launch_bytetests(relative != 0, p.d_mat, p.stride, c->n_pkts, c->d_bytetests, c->n_bt, rel_idx, c->n_bt_rel, c->bt_reach,
                                        c->d_patterns, c->d_arena, c->d_fold, c->d_off, c->d_len, c->d_windows, c->whole_payload != 0,
                                        (uint32_t)c->cu_count * 8u, f.d_rows, f.d_pc, f.d_any, c->stream);
        }));
        ++*launches;
    }
    return KMPGPU_OK;
}

/* The regex kernels behind a marking pass, in the same way: the linear one where an expression lacks KMPGPU_RX_GROUPS, then the grouped
 * one where an expression carries it.  *launches: how many that were. */
int enqueue_regexes(kmpgpu_ctx *c, const MarkPass &p, uint32_t *launches)
{
    FamilyRows f;
    family_rows(c, p, FAMILY_REGEXES, &f);
    if (c->n_rx_groups < c->n_rx) {
        HIP_TRY(profiled(c, [&] {
            return kmp_launch_regexes(p.d_mat, p.stride, c->n_pkts, c->d_regexes, c->n_rx, c->d_arena, c->d_off, c->d_len, c->whole_payload != 0,
                                      f.d_rows, f.d_pc, f.d_any, c->stream);
        }));
        ++*launches;
    }
    if (c->n_rx_groups) {
        HIP_TRY(profiled(c, [&] {
            return kmp_launch_regex_groups(p.d_mat, p.stride, c->n_pkts, c->d_regex_groups, c->n_rx_groups, c->d_arena, c->d_off, c->d_len,
                                           c->whole_payload != 0, f.d_rows, f.d_pc, f.d_any, c->stream);
        }));
        ++*launches;
    }
    return KMPGPU_OK;
}

/* The links behind a marking pass: the link buffer as kmpgpu_link_rows left it, copied into the links' rows of the matrix -- one
 * device-to-device copy, none while no link is filled (the pass has zeroed the rows).  reduce: their popcounts and their OR into any[] as
 * well, by the reduce of kmpgpu_scan_packets (kmpgpu_scan_links; the rules have no use for either).  *launches: the reduce, where it ran. */
int enqueue_links(kmpgpu_ctx *c, const MarkPass &p, bool reduce, uint32_t *launches)
{
    FamilyRows f;
    family_rows(c, p, FAMILY_LINKS, &f);
    if (c->n_links_filled == 0) return KMPGPU_OK;
    HIP_TRY(hipMemcpyAsync(f.d_rows, c->d_links, (size_t)(f.n_rows * p.stride) * sizeof(unsigned long long), hipMemcpyDeviceToDevice, c->stream));
    if (!reduce) return KMPGPU_OK;
    HIP_TRY(kmp_launch_marks_reduce(f.d_rows, (uint32_t)f.n_rows, p.stride, f.d_pc, f.d_any, c->stream));
    ++*launches;
    return KMPGPU_OK;
}

/* The one place that runs a family's kernels behind a marking pass, and says where they leave their results.  Patterns: the marks reduce.
 * Relations, chains, header predicates, byte tests, expressions: their kernels.  Links: the copy of their buffer.  Rules: the relation
 * kernel, the chain kernel, the header kernel, the byte-test kernels, the regex kernel and the links' copy where those are set, then the
 * rules kernel, into the context's rule buffer, grown here. */
int enqueue_family(kmpgpu_ctx *c, const char *who, int family, const MarkPass &p, bool profile_reduce, FamilyRows *f)
{
    hipEvent_t e1 = nullptr;
    if (family == KMPGPU_ALERT_PATTERNS) {
        family_rows(c, p, family, f);
        /* profile_reduce: kmpgpu_scan_alerts has a running profile record the marks reduce, kmpgpu_scan_packets never has */
        if (profile_reduce) HIP_TRY(profile_launch(c, &e1));
        HIP_TRY(kmp_launch_marks_reduce(p.d_mat, c->n_pat, p.stride, f->d_pc, f->d_any, c->stream));
        HIP_TRY(profile_launched(c, e1));
        f->launches = 1u;
        return KMPGPU_OK;
    }
    if (family == KMPGPU_ALERT_RULES) {
        const uint64_t nr = c->n_rules, words = nr * p.stride + nr + p.stride;
        hipError_t e = grow_buffer(&c->d_rule_out, &c->rule_out_cap, words, EIGHTH);
        if (e != hipSuccess) {
            /* the marking pass is under way on the stream; the context stays usable */
            (void)hipStreamSynchronize(c->stream);
            return alloc_fail(e, "%s: the rule rows (%llu bytes) could not be allocated", who, (unsigned long long)(words * 8u));
        }
        family_rows(c, p, family, f);
        /* the kernel adds to the counts and ORs into any; it writes every word of the rows itself */
        HIP_TRY(hipMemsetAsync(f->d_pc, 0, (size_t)(nr + p.stride) * sizeof(unsigned long long), c->stream));
        /* relations set: their rows of the matrix first, the rules read them as they read the patterns'; and so the chains' behind those */
        for (int pairing : {KMPGPU_ALERT_RELATIONS, KMPGPU_ALERT_CHAINS})
            if (family_n_rows(c, pairing)) {
                const int rr = enqueue_pairing(c, p, pairing);
                if (rr) return rr;
                f->launches++;
            }
        if (c->n_hdr) {
            const int rr = enqueue_headers(c, p);
            if (rr) return rr;
            f->launches++;
        }
        if (c->n_bt) {
            const int rr = enqueue_bytetests(c, p, &f->launches);
            if (rr) return rr;
        }
        if (c->n_rx) {
            const int rr = enqueue_regexes(c, p, &f->launches);
            if (rr) return rr;
        }
        if (c->n_links) {
            const int rr = enqueue_links(c, p, /* reduce = */ false, &f->launches);
            if (rr) return rr;
        }
        HIP_TRY(profiled(c, [&] {
            return kmp_launch_rules(p.d_mat, p.stride, c->n_pkts, c->d_rule_heads, c->d_rule_quads, c->n_rules, f->d_rows, f->d_pc, f->d_any, c->stream);
        }));
        f->launches++;
        return KMPGPU_OK;
    }
    family_rows(c, p, family, f);
    if (family == FAMILY_BYTETESTS) return enqueue_bytetests(c, p, &f->launches);
    if (family == FAMILY_REGEXES) return enqueue_regexes(c, p, &f->launches);
    if (family == FAMILY_LINKS) return enqueue_links(c, p, /* reduce = */ true, &f->launches);
    f->launches = 1u;
    return family == FAMILY_HEADERS ? enqueue_headers(c, p) : enqueue_pairing(c, p, family);
}

/* What every family's call starts with: the marking pass, and on an empty arena (p->empty) the outputs that hold something -- every payload
 * count, every total is 0, and there are no bit words. */
int begin_family(kmpgpu_ctx *c, const char *who, int family, uint64_t *row_counts_out, uint64_t *counts_out, kmpgpu_timing *t, MarkPass *p)
{
    /* header predicates are decided from the metadata: none on the context is found out before anything is launched */
    if ((family == FAMILY_HEADERS || (family == KMPGPU_ALERT_RULES && c->n_hdr)) && c->n_pkts && !c->has_meta)
        return fail(KMPGPU_ESTATE, "%s: no packet metadata (KMPGPU_OPT_KEEP_META, kmpgpu_set_meta)", who);
    /* ... and a rule over a link nobody has filled for this arena has no verdict to read */
    if (family == KMPGPU_ALERT_RULES)
        for (uint32_t q : c->rule_links)
            if (!c->link_filled[q]) return fail(KMPGPU_ESTATE, "%s: a rule names link %u, which is not filled (kmpgpu_link_rows)", who, q);
    const int rc = marking_pass(c, who, p);
    if (rc || !p->empty) return rc;
    if (row_counts_out) memset(row_counts_out, 0, (size_t)family_n_rows(c, family) * sizeof(uint64_t));
    if (counts_out) memset(counts_out, 0, (size_t)c->n_pat * sizeof(uint64_t));
    if (t) { *t = kmpgpu_timing{}; }
    return KMPGPU_OK;
}

/* waits for the pass and its downloads; kernel_ms = ev[0]..ev[1], d2h_ms = ev[1]..ev[2] */
int finish_marking(kmpgpu_ctx *c, uint32_t launches, kmpgpu_timing *t)
{
    HIP_TRY(hipEventRecord(c->ev[2], c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (t) {
        float k_ms = 0, d_ms = 0;
        HIP_TRY(hipEventElapsedTime(&k_ms, c->ev[0], c->ev[1]));
        HIP_TRY(hipEventElapsedTime(&d_ms, c->ev[1], c->ev[2]));
        *t = kmpgpu_timing{};
        t->kernel_ms = k_ms; t->d2h_ms = d_ms; t->launches = launches;
        t->grid_blocks = grid_blocks(c, primary_set(c), true);
    }
    return KMPGPU_OK;
}

/* The body of kmpgpu_scan_packets, _rules, _relations, _chains, _headers, _bytetests, _regexes and _links behind their own checks: marking pass, the family's kernels, downloads. */
int scan_family(kmpgpu_ctx *c, const char *who, int family, uint64_t *row_counts_out, uint64_t *any_out, uint64_t *hits_out, uint64_t *counts_out,
                kmpgpu_timing *t)
{
    MarkPass p;
    const int rc = begin_family(c, who, family, row_counts_out, counts_out, t, &p);
    if (rc || p.empty) return rc;
    FamilyRows f;
    const int rr = enqueue_family(c, who, family, p, /* profile_reduce = */ false, &f);
    if (rr) return rr;
    HIP_TRY(hipEventRecord(c->ev[1], c->stream));
    if (row_counts_out) HIP_TRY(hipMemcpyAsync(row_counts_out, f.d_pc, (size_t)f.n_rows * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    if (any_out) HIP_TRY(hipMemcpyAsync(any_out, f.d_any, p.W * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    if (counts_out) HIP_TRY(hipMemcpyAsync(counts_out, p.d_cnt, (size_t)c->n_pat * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    if (hits_out) HIP_TRY(download_rows(c, hits_out, f.d_rows, p.W, p.stride, f.n_rows));
    return finish_marking(c, p.launches + f.launches, t);
}

/* One table a setter swaps in: its words as a packer of kmp_rowtables.h left them (none: the table is cleared) and the context's pointer. */
struct HostTable {
    const std::vector<uint32_t> &words;
    void **slot;
};

/* The one place a table of the rules, windows, relations or chains reaches the device: every table into a fresh buffer, then the stream
 * synchronised (the words are the caller's locals, and no pass may still read an old table), then the old buffers freed and the new ones
 * in their place.  All or nothing: on failure the context is as it was. */
int swap_tables(kmpgpu_ctx *c, const char *what, std::initializer_list<HostTable> tables)
{
    std::vector<void *> fresh;
    hipError_t e = hipSuccess;
    for (const HostTable &tb : tables) {
        const size_t bytes = tb.words.size() * sizeof(uint32_t);
        fresh.push_back(nullptr);
        if (e == hipSuccess && bytes) e = hipMalloc(&fresh.back(), bytes);
        if (e == hipSuccess && bytes) e = hipMemcpyAsync(fresh.back(), tb.words.data(), bytes, hipMemcpyHostToDevice, c->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        for (void *d : fresh) free_buffer(&d);
        return alloc_fail(e, "%s could not be uploaded", what);
    }
    size_t k = 0;
    for (const HostTable &tb : tables) {
        free_buffer(tb.slot);
        *tb.slot = fresh[k++];
    }
    return KMPGPU_OK;
}

/* what every setter checks before it looks at its table */
int setter_state(kmpgpu_ctx *c, const char *who)
{
    if (!c) return fail(KMPGPU_EINVAL, "%s: ctx is NULL", who);
    if (!c->d_patterns || c->n_pat == 0) return fail(KMPGPU_ESTATE, "%s: no patterns set", who);
    HIP_TRY(hipSetDevice(c->device));
    return KMPGPU_OK;
}

/* The links sit behind every other family and have no table of their own, so no packer counts them: a setter that grows a family in front
 * of them holds the sum below the 2^31 rows a rule term can name itself.  rows: what the context would hold without the links. */
int links_fit(const kmpgpu_ctx *c, const char *who, uint64_t rows)
{
    if (c->n_links && rows + c->n_links >= (1ull << 31))
        return fail(KMPGPU_EINVAL, "%s: %llu rows + %u links do not fit the 2^31 rows a rule term can name", who, (unsigned long long)rows, c->n_links);
    return KMPGPU_OK;
}

}  // namespace

int kmpgpu_scan_packets(kmpgpu_ctx *c, uint64_t *pkt_counts_out, uint64_t *any_out, uint64_t *hits_out, uint64_t *counts_out, kmpgpu_timing *t)
{
    if (!c) return fail(KMPGPU_EINVAL, "kmpgpu_scan_packets: ctx is NULL");
    return scan_family(c, "kmpgpu_scan_packets", KMPGPU_ALERT_PATTERNS, pkt_counts_out, any_out, hits_out, counts_out, t);
}

int kmpgpu_set_rules(kmpgpu_ctx *c, const uint32_t *rule_off, const uint32_t *terms, uint32_t n_rules)
{
    const int sr = setter_state(c, "kmpgpu_set_rules");
    if (sr) return sr;
    std::vector<uint32_t> heads, quads, named;
    std::string msg;
    if (n_rules) {
        const int rc = kmp_pack_rules(rule_off, terms, n_rules, c->n_pat, c->n_rel, c->n_chains, c->n_hdr, c->n_bt, c->n_rx, c->n_links, &heads, &quads, &msg);
        if (rc) return fail(rc, "%s", msg.c_str());
        if (quads.empty()) quads.assign(4, 0u);         /* rules of one or two terms only: one quad nobody reads, never a NULL table */
        /* which links the rules name: what every rules pass checks for filled rows before it starts */
        const uint32_t link0 = c->n_pat + c->n_rel + c->n_chains + c->n_hdr + c->n_bt + c->n_rx;
        for (uint32_t j = 0; j < rule_off[n_rules] && c->n_links; j++)
            if ((terms[j] & ~KMPGPU_RULE_NOT) >= link0) named.push_back((terms[j] & ~KMPGPU_RULE_NOT) - link0);
        std::sort(named.begin(), named.end());
        named.erase(std::unique(named.begin(), named.end()), named.end());
    }
    const int rc = swap_tables(c, "kmpgpu_set_rules: the rules", {{heads, (void **)&c->d_rule_heads}, {quads, (void **)&c->d_rule_quads}});
    if (rc) return rc;
    c->n_rules = n_rules;
    c->rule_links.swap(named);
    drop_flowbits(c);                              /* their rule indices meant the rules before */
    drop_thresholds(c);
    return KMPGPU_OK;
}

int kmpgpu_set_windows(kmpgpu_ctx *c, const uint32_t *first, const uint32_t *last, uint32_t n_pat)
{
    const int sr = setter_state(c, "kmpgpu_set_windows");
    if (sr) return sr;
    std::vector<uint32_t> win;
    std::string msg;
    if (n_pat) {
        const int rc = kmp_pack_windows(first, last, n_pat, c->n_pat, &win, &msg);
        if (rc) return fail(rc, "%s", msg.c_str());
    }
    return swap_tables(c, "kmpgpu_set_windows: the windows", {{win, (void **)&c->d_windows}});
}

int kmpgpu_scan_rules(kmpgpu_ctx *c, uint64_t *rule_pkt_counts_out, uint64_t *any_out, uint64_t *rule_hits_out, uint64_t *counts_out, kmpgpu_timing *t)
{
    if (!c) return fail(KMPGPU_EINVAL, "kmpgpu_scan_rules: ctx is NULL");
    if (c->n_rules == 0) return fail(KMPGPU_ESTATE, "kmpgpu_scan_rules: no rules set");
    return scan_family(c, "kmpgpu_scan_rules", KMPGPU_ALERT_RULES, rule_pkt_counts_out, any_out, rule_hits_out, counts_out, t);
}

int kmpgpu_set_relations(kmpgpu_ctx *c, const kmpgpu_relation *rel, uint32_t n_rel)
{
    const int sr = setter_state(c, "kmpgpu_set_relations");
    if (sr) return sr;
    const int lf = links_fit(c, "kmpgpu_set_relations", (uint64_t)c->n_pat + n_rel + c->n_chains + c->n_hdr + c->n_bt + c->n_rx);
    if (lf) return lf;
    std::vector<uint32_t> host;
    std::string msg;
    if (n_rel) {
        const int rc = kmp_pack_relations(rel, n_rel, c->n_pat, c->n_chains, c->n_hdr, c->n_bt, c->n_rx, c->pat_fold.data(), &host, &msg);
        if (rc) return fail(rc, "%s", msg.c_str());
    }
    const int rc = swap_tables(c, "kmpgpu_set_relations: the relations", {{host, (void **)&c->d_relations}});
    if (rc) return rc;
    drop_rules(c);                                 /* the rows their terms named are no longer the same, whatever was set or cleared */
    c->n_rel = n_rel;
    return KMPGPU_OK;
}

int kmpgpu_scan_relations(kmpgpu_ctx *c, uint64_t *rel_pkt_counts_out, uint64_t *any_out, uint64_t *rel_hits_out, uint64_t *counts_out, kmpgpu_timing *t)
{
    if (!c) return fail(KMPGPU_EINVAL, "kmpgpu_scan_relations: ctx is NULL");
    if (!c->d_patterns || c->n_pat == 0) return fail(KMPGPU_ESTATE, "kmpgpu_scan_relations: no patterns set");
    if (c->n_rel == 0) return fail(KMPGPU_ESTATE, "kmpgpu_scan_relations: no relations set");
    return scan_family(c, "kmpgpu_scan_relations", KMPGPU_ALERT_RELATIONS, rel_pkt_counts_out, any_out, rel_hits_out, counts_out, t);
}

int kmpgpu_set_chains(kmpgpu_ctx *c, const uint32_t *chain_off, const kmpgpu_chain_link *links, uint32_t n_chains)
{
    const int sr = setter_state(c, "kmpgpu_set_chains");
    if (sr) return sr;
    const int lf = links_fit(c, "kmpgpu_set_chains", (uint64_t)c->n_pat + c->n_rel + n_chains + c->n_hdr + c->n_bt + c->n_rx);
    if (lf) return lf;
    std::vector<uint32_t> host;
    std::string msg;
    if (n_chains) {
        const int rc = kmp_pack_chains(chain_off, links, n_chains, c->n_pat, c->n_rel, c->n_hdr, c->n_bt, c->n_rx, c->pat_fold.data(), &host, &msg);
        if (rc) return fail(rc, "%s", msg.c_str());
    }
    const int rc = swap_tables(c, "kmpgpu_set_chains: the chains", {{host, (void **)&c->d_chains}});
    if (rc) return rc;
    drop_rules(c);                                 /* the rows their terms named are no longer the same, whatever was set or cleared */
    c->n_chains = n_chains;
    return KMPGPU_OK;
}

int kmpgpu_scan_chains(kmpgpu_ctx *c, uint64_t *chain_pkt_counts_out, uint64_t *any_out, uint64_t *chain_hits_out, uint64_t *counts_out, kmpgpu_timing *t)
{
    if (!c) return fail(KMPGPU_EINVAL, "kmpgpu_scan_chains: ctx is NULL");
    if (!c->d_patterns || c->n_pat == 0) return fail(KMPGPU_ESTATE, "kmpgpu_scan_chains: no patterns set");
    if (c->n_chains == 0) return fail(KMPGPU_ESTATE, "kmpgpu_scan_chains: no chains set");
    return scan_family(c, "kmpgpu_scan_chains", KMPGPU_ALERT_CHAINS, chain_pkt_counts_out, any_out, chain_hits_out, counts_out, t);
}

int kmpgpu_set_headers(kmpgpu_ctx *c, const kmpgpu_header *h, uint32_t n_hdr)
{
    static_assert(sizeof(kmpgpu_header) == 36, "kmpgpu_header is the 36-byte record of kmpgpu.h");
    const int sr = setter_state(c, "kmpgpu_set_headers");
    if (sr) return sr;
    const int lf = links_fit(c, "kmpgpu_set_headers", (uint64_t)c->n_pat + c->n_rel + c->n_chains + n_hdr + c->n_bt + c->n_rx);
    if (lf) return lf;
    std::vector<uint32_t> host;
    std::string msg;
    if (n_hdr) {
        const int rc = kmp_pack_headers(h, n_hdr, c->n_pat, c->n_rel, c->n_chains, c->n_bt, c->n_rx, &host, &msg);
        if (rc) return fail(rc, "%s", msg.c_str());
    }
    const int rc = swap_tables(c, "kmpgpu_set_headers: the header predicates", {{host, (void **)&c->d_headers}});
    if (rc) return rc;
    drop_rules(c);                                 /* the rows their terms named are no longer the same, whatever was set or cleared */
    c->n_hdr = n_hdr;
    return KMPGPU_OK;
}

int kmpgpu_scan_headers(kmpgpu_ctx *c, uint64_t *hdr_pkt_counts_out, uint64_t *any_out, uint64_t *hdr_hits_out, uint64_t *counts_out, kmpgpu_timing *t)
{
    if (!c) return fail(KMPGPU_EINVAL, "kmpgpu_scan_headers: ctx is NULL");
    if (!c->d_patterns || c->n_pat == 0) return fail(KMPGPU_ESTATE, "kmpgpu_scan_headers: no patterns set");
    if (c->n_hdr == 0) return fail(KMPGPU_ESTATE, "kmpgpu_scan_headers: no header predicates set");
    return scan_family(c, "kmpgpu_scan_headers", FAMILY_HEADERS, hdr_pkt_counts_out, any_out, hdr_hits_out, counts_out, t);
}

int kmpgpu_set_bytetests(kmpgpu_ctx *c, const kmpgpu_bytetest *bt, uint32_t n_bt)
{
    static_assert(sizeof(kmpgpu_bytetest) == 20, "kmpgpu_bytetest is the 20-byte record of kmpgpu.h");
    const int sr = setter_state(c, "kmpgpu_set_bytetests");
    if (sr) return sr;
    const int lf = links_fit(c, "kmpgpu_set_bytetests", (uint64_t)c->n_pat + c->n_rel + c->n_chains + c->n_hdr + n_bt + c->n_rx);
    if (lf) return lf;
    std::vector<uint32_t> host;
    std::string msg;
    uint32_t n_relative = 0, reach = 0;
    if (n_bt) {
        const int rc = kmp_pack_bytetests(bt, n_bt, c->n_pat, c->n_rel, c->n_chains, c->n_hdr, c->n_rx, c->pat_fold.data(), &host, &n_relative, &reach, &msg);
        if (rc) return fail(rc, "%s", msg.c_str());
    }
    const int rc = swap_tables(c, "kmpgpu_set_bytetests: the byte tests", {{host, (void **)&c->d_bytetests}});
    if (rc) return rc;
    drop_rules(c);                                 /* the rows their terms named are no longer the same, whatever was set or cleared */
    c->n_bt = n_bt; c->n_bt_rel = n_relative; c->bt_reach = reach;
    return KMPGPU_OK;
}

int kmpgpu_scan_bytetests(kmpgpu_ctx *c, uint64_t *bt_pkt_counts_out, uint64_t *any_out, uint64_t *bt_hits_out, uint64_t *counts_out, kmpgpu_timing *t)
{
    if (!c) return fail(KMPGPU_EINVAL, "kmpgpu_scan_bytetests: ctx is NULL");
    if (!c->d_patterns || c->n_pat == 0) return fail(KMPGPU_ESTATE, "kmpgpu_scan_bytetests: no patterns set");
    if (c->n_bt == 0) return fail(KMPGPU_ESTATE, "kmpgpu_scan_bytetests: no byte tests set");
    return scan_family(c, "kmpgpu_scan_bytetests", FAMILY_BYTETESTS, bt_pkt_counts_out, any_out, bt_hits_out, counts_out, t);
}

int kmpgpu_set_regexes(kmpgpu_ctx *c, const uint8_t *const *expr, const uint32_t *expr_len, const uint32_t *flags, const uint32_t *gate, uint32_t n_rx)
{
    const int sr = setter_state(c, "kmpgpu_set_regexes");
    if (sr) return sr;
    const int lf = links_fit(c, "kmpgpu_set_regexes", (uint64_t)c->n_pat + c->n_rel + c->n_chains + c->n_hdr + c->n_bt + n_rx);
    if (lf) return lf;
    std::vector<uint32_t> host, host_groups;
    std::string msg;
    uint32_t n_groups = 0;
    if (n_rx) {
        int rc = kmp_pack_regexes(expr, expr_len, flags, gate, n_rx, c->n_pat, c->n_rel, c->n_chains, c->n_hdr, c->n_bt, &host, &msg);
        if (!rc) rc = kmp_pack_regex_groups(expr, expr_len, flags, gate, n_rx, c->n_pat, c->n_rel, c->n_chains, c->n_hdr, c->n_bt, &host_groups, &n_groups, &msg);
        if (rc) return fail(rc, "%s", msg.c_str());
    }
    /* both tables or neither */
    const int rc = swap_tables(c, "kmpgpu_set_regexes: the expressions", {{host, (void **)&c->d_regexes}, {host_groups, (void **)&c->d_regex_groups}});
    if (rc) return rc;
    drop_rules(c);                                 /* the rows their terms named are no longer the same, whatever was set or cleared */
    c->n_rx = n_rx;
    c->n_rx_groups = n_groups;
    return KMPGPU_OK;
}

int kmpgpu_scan_regexes(kmpgpu_ctx *c, uint64_t *rx_pkt_counts_out, uint64_t *any_out, uint64_t *rx_hits_out, uint64_t *counts_out, kmpgpu_timing *t)
{
    if (!c) return fail(KMPGPU_EINVAL, "kmpgpu_scan_regexes: ctx is NULL");
    if (!c->d_patterns || c->n_pat == 0) return fail(KMPGPU_ESTATE, "kmpgpu_scan_regexes: no patterns set");
    if (c->n_rx == 0) return fail(KMPGPU_ESTATE, "kmpgpu_scan_regexes: no expressions set");
    return scan_family(c, "kmpgpu_scan_regexes", FAMILY_REGEXES, rx_pkt_counts_out, any_out, rx_hits_out, counts_out, t);
}

int kmpgpu_set_links(kmpgpu_ctx *c, uint32_t n_links)
{
    const int sr = setter_state(c, "kmpgpu_set_links");
    if (sr) return sr;
    if ((uint64_t)c->n_pat + c->n_rel + c->n_chains + c->n_hdr + c->n_bt + c->n_rx + n_links >= (1ull << 31))
        return fail(KMPGPU_EINVAL, "kmpgpu_set_links: %u links behind the %llu rows in front of them do not fit the 2^31 rows a rule term can name", n_links,
                    (unsigned long long)c->n_pat + c->n_rel + c->n_chains + c->n_hdr + c->n_bt + c->n_rx);
    HIP_TRY(hipStreamSynchronize(c->stream));      /* no pass may still copy the old rows */
    drop_rules(c);                                 /* the rows their terms named are no longer the same, whatever was set or cleared */
    drop_links(c);
    c->n_links = n_links;
    c->link_filled.assign(n_links, (uint8_t)0);
    return KMPGPU_OK;
}

int kmpgpu_link_rows(kmpgpu_ctx *dst, uint32_t first_link, kmpgpu_ctx *src, int family, uint32_t first_row, uint32_t n_rows, int map_kind,
                     const void *map, int map_on_device, kmpgpu_timing *t)
{
    const char *who = "kmpgpu_link_rows";
    if (!dst || !src) return fail(KMPGPU_EINVAL, "%s: ctx is NULL", who);
    if (dst == src) return fail(KMPGPU_EINVAL, "%s: dst and src are the same context (links to a context's own rows do not exist)", who);
    if (dst->device != src->device)
        return fail(KMPGPU_EINVAL, "%s: the contexts sit on devices %d and %d (links across devices do not exist)", who, dst->device, src->device);
    if (family < KMPGPU_ALERT_PATTERNS || family > KMPGPU_ALERT_CHAINS) return fail(KMPGPU_EINVAL, "%s: family %d is none of KMPGPU_ALERT_*", who, family);
    if (map_kind != KMPGPU_LINK_SAME && map_kind != KMPGPU_LINK_BITMAP && map_kind != KMPGPU_LINK_INDEX)
        return fail(KMPGPU_EINVAL, "%s: map kind %d is none of KMPGPU_LINK_*", who, map_kind);
    if (map_on_device != 0 && map_on_device != 1) return fail(KMPGPU_EINVAL, "%s: map_on_device is %d, not 0 or 1", who, map_on_device);
    const uint64_t src_rows = family_n_rows(src, family);
    if ((uint64_t)first_row + n_rows > src_rows)
        return fail(KMPGPU_EINVAL, "%s: rows %u .. %llu of the %llu rows of src's family %d", who, first_row, (unsigned long long)first_row + n_rows, (unsigned long long)src_rows, family);
    if ((uint64_t)first_link + n_rows > dst->n_links)
        return fail(KMPGPU_EINVAL, "%s: links %u .. %llu of dst's %u links", who, first_link, (unsigned long long)first_link + n_rows, dst->n_links);
    const uint64_t n_dst = dst->n_pkts, n_src = src->n_pkts;
    if (map_kind == KMPGPU_LINK_SAME && n_src != n_dst)
        return fail(KMPGPU_EINVAL, "%s: KMPGPU_LINK_SAME between %llu payloads of src and %llu of dst", who, (unsigned long long)n_src, (unsigned long long)n_dst);
    if (map_kind != KMPGPU_LINK_SAME && n_dst && !map) return fail(KMPGPU_EINVAL, "%s: map is NULL", who);
    if (map_kind != KMPGPU_LINK_SAME && map_on_device && ((uintptr_t)map & (map_kind == KMPGPU_LINK_BITMAP ? 7u : 3u)))
        return fail(KMPGPU_EINVAL, "%s: the device map is not %d-byte aligned", who, map_kind == KMPGPU_LINK_BITMAP ? 8 : 4);
    if (dst->fr_pending || src->fr_pending)
        return fail(KMPGPU_ESTATE, "%s: %s sits between kmpgpu_load_frames_begin and _finish", who, dst->fr_pending ? "dst" : "src");
    if (dst->n_links == 0) return fail(KMPGPU_ESTATE, "%s: dst: no links set", who);
    if (!dst->d_off || n_dst == 0) return fail(KMPGPU_ESTATE, "%s: dst has no arena loaded", who);
    /* what src's own call for the family refuses before it launches anything (the marking pass says the rest) */
    if (!src->d_patterns || src->n_pat == 0) return fail(KMPGPU_ESTATE, "%s: src: no patterns set", who);
    if (family != KMPGPU_ALERT_PATTERNS && src_rows == 0)
        return fail(KMPGPU_ESTATE, "%s: src: no %s set", who, family == KMPGPU_ALERT_RULES ? "rules" : family == KMPGPU_ALERT_RELATIONS ? "relations" : "chains");
    if (n_dst > 0xFFFFFFFFull && map_kind == KMPGPU_LINK_INDEX) return fail(KMPGPU_EINVAL, "%s: too many payloads for a 32-bit index map", who);
    HIP_TRY(hipSetDevice(dst->device));
    HIP_TRY(hipStreamSynchronize(dst->stream));           /* the passes that still copy the link rows */
    HIP_TRY(hipStreamSynchronize(src->stream));
    kmpgpu_ctx *c = dst;
    const uint64_t W = (n_dst + 63u) / 64u, stride = (W + 1u) & ~1ull;
    uint32_t launches = 0;

    /* the map on the device, and a bitmap's ranks; their total is checked before a word of a link is written */
    const uint64_t map_bytes = map_kind == KMPGPU_LINK_BITMAP ? W * sizeof(uint64_t) : map_kind == KMPGPU_LINK_INDEX ? n_dst * sizeof(uint32_t) : 0u;
    const uint64_t up_bytes = map_on_device ? 0u : (map_bytes + 15u) & ~15ull;
    const uint64_t rank_bytes = map_kind == KMPGPU_LINK_BITMAP ? kmp_link_rank_bytes(n_dst) : 0u;
    if (up_bytes + rank_bytes) {
        const hipError_t e = grow_buffer(&c->d_link_ws, &c->link_ws_cap, up_bytes + rank_bytes, EIGHTH);
        if (e != hipSuccess) return alloc_fail(e, "%s: the map's workspace (%llu bytes) could not be allocated", who, (unsigned long long)(up_bytes + rank_bytes));
    }
    const void *d_map = map;
    if (map_kind != KMPGPU_LINK_SAME && !map_on_device) {
        HIP_TRY(hipMemcpyAsync(c->d_link_ws, map, (size_t)map_bytes, hipMemcpyHostToDevice, c->stream));
        d_map = c->d_link_ws;
    }
    uint8_t *rank_ws = c->d_link_ws + up_bytes;
    if (map_kind == KMPGPU_LINK_BITMAP) {
        HIP_TRY(hipEventRecord(c->ev[2], c->stream));
        HIP_TRY(kmp_launch_link_rank((const unsigned long long *)d_map, n_dst, rank_ws, c->stream));
        HIP_TRY(hipEventRecord(c->ev[3], c->stream));
        launches += 2u;
        HIP_TRY(hipMemcpyAsync(c->h_small, kmp_link_rank_total(rank_ws, n_dst), sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));     /* (pinned: no staging) */
        HIP_TRY(hipStreamSynchronize(c->stream));
        const unsigned long long total = c->h_small[0];
        if (total != n_src)
            return fail(KMPGPU_EINVAL, "%s: the bitmap has %llu bits set below dst's %llu payloads, src holds %llu payloads", who, total,
                        (unsigned long long)n_dst, (unsigned long long)n_src);
    }

    /* src's pass: the body of scan_family without a download */
    MarkPass p;
    FamilyRows f;
    const int rc = begin_family(src, who, family, nullptr, nullptr, nullptr, &p);
    if (rc) return rc;
    if (!p.empty) {
        const int rr = enqueue_family(src, who, family, p, /* profile_reduce = */ false, &f);
        if (rr) return rr;
        HIP_TRY(hipEventRecord(src->ev[1], src->stream));
        const int fr = finish_marking(src, p.launches + f.launches, nullptr);
        if (fr) return fr;
    }

    /* dst's link buffer: taken anew for another stride (no link is filled then), all zero while no link is filled */
    const uint64_t words = (uint64_t)c->n_links * stride;
    if (c->n_links_filled == 0) {
        const hipError_t e = grow_buffer(&c->d_links, &c->links_cap, words, EIGHTH);
        if (e != hipSuccess) return alloc_fail(e, "%s: the link rows (%llu bytes) could not be allocated", who, (unsigned long long)(words * 8u));
        c->links_stride = stride;
        HIP_TRY(hipMemsetAsync(c->d_links, 0, (size_t)words * sizeof(unsigned long long), c->stream));
    }
    unsigned long long *d_out = c->d_links + (uint64_t)first_link * stride;
    HIP_TRY(hipEventRecord(c->ev[0], c->stream));              /* (behind src's pass: the translation's own time) */
    if (p.empty) {
        /* src without payloads: no row has a bit */
        if (n_rows) HIP_TRY(hipMemsetAsync(d_out, 0, (size_t)((uint64_t)n_rows * stride) * sizeof(unsigned long long), c->stream));
    } else if (n_rows) {
        HIP_TRY(kmp_launch_link_gather(map_kind, f.d_rows + (uint64_t)first_row * p.stride, p.stride, n_src, n_rows, n_dst, d_map, rank_ws, d_out, stride,
                                       c->stream));
        launches += 1u;
    }
    HIP_TRY(hipEventRecord(c->ev[1], c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (uint32_t q = first_link; q < first_link + n_rows; q++)
        if (!c->link_filled[q]) { c->link_filled[q] = 1; c->n_links_filled++; }
    if (t) {
        float ms = 0, rank_ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
        if (map_kind == KMPGPU_LINK_BITMAP) HIP_TRY(hipEventElapsedTime(&rank_ms, c->ev[2], c->ev[3]));
        *t = kmpgpu_timing{};
        t->kernel_ms = ms + rank_ms; t->launches = launches;
    }
    return KMPGPU_OK;
}

int kmpgpu_scan_links(kmpgpu_ctx *c, uint64_t *link_pkt_counts_out, uint64_t *any_out, uint64_t *link_hits_out, uint64_t *counts_out, kmpgpu_timing *t)
{
    if (!c) return fail(KMPGPU_EINVAL, "kmpgpu_scan_links: ctx is NULL");
    if (!c->d_patterns || c->n_pat == 0) return fail(KMPGPU_ESTATE, "kmpgpu_scan_links: no patterns set");
    if (c->n_links == 0) return fail(KMPGPU_ESTATE, "kmpgpu_scan_links: no links set");
    return scan_family(c, "kmpgpu_scan_links", FAMILY_LINKS, link_pkt_counts_out, any_out, link_hits_out, counts_out, t);
}

int kmpgpu_set_meta(kmpgpu_ctx *c, const void *meta, uint64_t n_pkts, int on_device)
{
    static_assert(sizeof(kmpgpu_pkt_meta) == 16, "kmpgpu_pkt_meta is the 16-byte record of kmpgpu.h");
    if (!c) return fail(KMPGPU_EINVAL, "kmpgpu_set_meta: ctx is NULL");
    if (on_device != 0 && on_device != 1) return fail(KMPGPU_EINVAL, "kmpgpu_set_meta: on_device is %d, not 0 or 1", on_device);
    if (c->fr_pending) return fail(KMPGPU_ESTATE, "kmpgpu_set_meta: the context sits between kmpgpu_load_frames_begin and _finish");
    if (n_pkts == 0 && !meta) { c->has_meta = false; drop_flows(c); return KMPGPU_OK; }
    if (!c->d_off || c->n_pkts == 0) return fail(KMPGPU_ESTATE, "kmpgpu_set_meta: no arena loaded");
    if (n_pkts != c->n_pkts)
        return fail(KMPGPU_EINVAL, "kmpgpu_set_meta: %llu records for the arena's %llu payloads", (unsigned long long)n_pkts, (unsigned long long)c->n_pkts);
    if (!meta) return fail(KMPGPU_EINVAL, "kmpgpu_set_meta: meta is NULL");
    if (on_device && ((uintptr_t)meta & 3u)) return fail(KMPGPU_EINVAL, "kmpgpu_set_meta: the device records are not 4-byte aligned");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));      /* a pass may still read the records that are about to be replaced */
    /* into a fresh buffer where the one at hand is too small: after a failure the metadata that was there stays */
    uint4 *d = c->d_meta;
    if (c->meta_cap < n_pkts) {
        const hipError_t e = hipMalloc((void **)&d, (size_t)n_pkts * sizeof(uint4));
        if (e != hipSuccess) return alloc_fail(e, "kmpgpu_set_meta: the metadata (%llu bytes) could not be allocated", (unsigned long long)(n_pkts * 16u));
    }
    hipError_t e = hipMemcpyAsync(d, meta, (size_t)n_pkts * sizeof(uint4), on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        if (d != c->d_meta) (void)hipFree(d); else { c->has_meta = false; drop_flows(c); }       /* (copied over in place: what was there is gone) */
        return alloc_fail(e, "kmpgpu_set_meta: the metadata could not be copied");
    }
    if (d != c->d_meta) { free_buffer(&c->d_meta, &c->meta_cap); c->d_meta = d; c->meta_cap = n_pkts; }
    c->has_meta = true;
    drop_flows(c);                                 /* they grouped the payloads by the records before these */
    return KMPGPU_OK;
}

int kmpgpu_meta_download(kmpgpu_ctx *c, kmpgpu_pkt_meta *out, uint64_t cap, uint64_t *n)
{
    if (!c) return fail(KMPGPU_EINVAL, "kmpgpu_meta_download: ctx is NULL");
    if (n) *n = 0;
    if (!c->has_meta) return fail(KMPGPU_ESTATE, "kmpgpu_meta_download: no packet metadata (KMPGPU_OPT_KEEP_META, kmpgpu_set_meta)");
    if (n) *n = c->n_pkts;
    if (!out || c->n_pkts == 0) return KMPGPU_OK;
    if (cap < c->n_pkts) return fail(KMPGPU_EINVAL, "kmpgpu_meta_download: room for %llu of %llu records", (unsigned long long)cap, (unsigned long long)c->n_pkts);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(out, c->d_meta, (size_t)c->n_pkts * sizeof(uint4), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return KMPGPU_OK;
}

int kmpgpu_scan_alerts(kmpgpu_ctx *c, int family, uint64_t max_records, uint64_t *n_found, uint64_t *n_packets, uint64_t *pkt_counts_out,
                       uint64_t *counts_out, kmpgpu_timing *t)
{
    static_assert(sizeof(kmpgpu_alert) == sizeof(uint4), "an alert is a 16-byte record");
    if (!c || !n_found) return fail(KMPGPU_EINVAL, "kmpgpu_scan_alerts: NULL argument");
    *n_found = 0;
    if (n_packets) *n_packets = 0;
    if (family < KMPGPU_ALERT_PATTERNS || family > KMPGPU_ALERT_CHAINS) return fail(KMPGPU_EINVAL, "kmpgpu_scan_alerts: family %d is none of KMPGPU_ALERT_*", family);
    /* the rows of the family, as its own call checks them (no patterns for the patterns' own: the marking pass says so) */
    const uint64_t n_rows = family_n_rows(c, family);
    if (family != KMPGPU_ALERT_PATTERNS && (!c->d_patterns || c->n_pat == 0)) return fail(KMPGPU_ESTATE, "kmpgpu_scan_alerts: no patterns set");
    if (family != KMPGPU_ALERT_PATTERNS && n_rows == 0)
        return fail(KMPGPU_ESTATE, "kmpgpu_scan_alerts: no %s set", family == KMPGPU_ALERT_RULES ? "rules" : family == KMPGPU_ALERT_RELATIONS ? "relations" : "chains");
    if (c->fr_pending) return fail(KMPGPU_ESTATE, "kmpgpu_scan_alerts: the context sits between kmpgpu_load_frames_begin and _finish");
    /* a payload's records are scanned as a 32-bit byte length (kmp_scan_local_kernel), 0xFFFFFFFF taken */
    if (16ull * n_rows > 0xFFFFFFFEull) return fail(KMPGPU_EINVAL, "kmpgpu_scan_alerts: %llu rows: 16 bytes x rows do not fit 32 bits", (unsigned long long)n_rows);
    c->alerts_valid = false;                       /* the list before this pass is gone, whatever happens */
    MarkPass p;
    const int rc = begin_family(c, "kmpgpu_scan_alerts", family, pkt_counts_out, counts_out, t, &p);
    if (rc) return rc;
    if (p.empty) {
        /* nothing to scan: an empty list */
        c->alerts_kept = 0; c->alerts_valid = true;
        return KMPGPU_OK;
    }
    /* the family's rows, their popcounts and their OR, by the kernels of the family's own call */
    FamilyRows f;
    const int rr = enqueue_family(c, "kmpgpu_scan_alerts", family, p, /* profile_reduce = */ true, &f);
    if (rr) return rr;
    uint32_t launches = p.launches + f.launches;
    /* the list: count, scan (in the scratch kept for kmpgpu_load_frames, as kmpgpu_load_selected uses it), the totals read once, fill */
    hipError_t e = grow_buffer(&c->fr_ws, &c->fr_ws_cap, (uint64_t)kmp_extract_ws_bytes(c->n_pkts), EIGHTH);
    if (e == hipSuccess && !c->fr_tot) e = hipMalloc(&c->fr_tot, 2 * sizeof(unsigned long long));
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(c->stream);      /* the pass is under way on the stream; the context stays usable */
        return alloc_fail(e, "kmpgpu_scan_alerts: the scan workspace (%llu bytes) could not be allocated", (unsigned long long)kmp_extract_ws_bytes(c->n_pkts));
    }
    HIP_TRY(profiled(c, [&] { return kmp_launch_alerts_count(f.d_rows, p.stride, (uint32_t)f.n_rows, c->n_pkts, f.d_any, c->fr_ws, c->stream); }));
    HIP_TRY(profiled(c, [&] { return kmp_launch_compact_scan(c->n_pkts, c->fr_ws, c->fr_tot, c->stream); }));
    HIP_TRY(hipMemcpyAsync(c->h_small, c->fr_tot, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));         /* (pinned: no staging) */
    HIP_TRY(hipStreamSynchronize(c->stream));
    unsigned long long tot[2] = {0, 0};
    memcpy(tot, c->h_small, sizeof tot);
    const uint64_t found = tot[0] / 16u, kept = std::min<uint64_t>(found, max_records);
    launches += 3u;
    if (kept) {
        e = grow_buffer(&c->d_alerts, &c->alerts_cap, kept, EIGHTH);
        if (e != hipSuccess) return alloc_fail(e, "kmpgpu_scan_alerts: the records (%llu bytes) could not be allocated", (unsigned long long)(kept * 16u));
        HIP_TRY(profiled(c, [&] { return kmp_launch_alerts_fill(f.d_rows, p.stride, (uint32_t)f.n_rows, c->n_pkts, f.d_any, c->fr_ws, c->d_alerts, kept, c->stream); }));
        launches += 1u;
    }
    HIP_TRY(hipEventRecord(c->ev[1], c->stream));
    if (pkt_counts_out) HIP_TRY(hipMemcpyAsync(pkt_counts_out, f.d_pc, (size_t)f.n_rows * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    if (counts_out) HIP_TRY(hipMemcpyAsync(counts_out, p.d_cnt, (size_t)c->n_pat * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    const int fr = finish_marking(c, launches, t);
    if (fr) return fr;
    *n_found = found;
    if (n_packets) *n_packets = tot[1];
    c->alerts_kept = kept; c->alerts_valid = true;
    return KMPGPU_OK;
}

int kmpgpu_alerts_read(kmpgpu_ctx *c, kmpgpu_alert *out, uint64_t first, uint64_t n)
{
    if (!c) return fail(KMPGPU_EINVAL, "kmpgpu_alerts_read: ctx is NULL");
    return read_range(c, "kmpgpu_alerts_read", c->alerts_valid, "no list (no kmpgpu_scan_alerts since the arena or the patterns were set)", out,
                      c->d_alerts, sizeof(kmpgpu_alert), first, n, c->alerts_kept, "records", "kept");
}

int kmpgpu_flows_build(kmpgpu_ctx *c, uint32_t flags, uint64_t *n_flows, kmpgpu_timing *t)
{
    static_assert(sizeof(kmpgpu_flow) == 48, "kmpgpu_flow is the 48-byte record of kmpgpu.h");
    if (!c) return fail(KMPGPU_EINVAL, "kmpgpu_flows_build: ctx is NULL");
    if (n_flows) *n_flows = 0;
    if (flags & ~KMPGPU_FLOW_DIRECTED) return fail(KMPGPU_EINVAL, "kmpgpu_flows_build: flags 0x%x hold a bit that is none of KMPGPU_FLOW_*", flags);
    if (c->fr_pending) return fail(KMPGPU_ESTATE, "kmpgpu_flows_build: the context sits between kmpgpu_load_frames_begin and _finish");
    const uint64_t n = c->n_pkts;
    if (n && !c->has_meta) return fail(KMPGPU_ESTATE, "kmpgpu_flows_build: no packet metadata (KMPGPU_OPT_KEEP_META, kmpgpu_set_meta)");
    if (n > 0xFFFFFFFEull) return fail(KMPGPU_EINVAL, "kmpgpu_flows_build: %llu payloads: flow ids are 32 bits wide", (unsigned long long)n);
    const uint64_t slots = c->flow_slots ? (uint64_t)c->flow_slots : kmp_flow_auto_slots(n);
    if ((slots & (slots - 1)) || slots <= n || slots > (1ull << 32))
        return fail(KMPGPU_EINVAL, "kmpgpu_flows_build: KMPGPU_OPT_FLOW_SLOTS is %llu, no power of two above the %llu payloads (at most 2^32)",
                    (unsigned long long)slots, (unsigned long long)n);
    drop_flows(c, /* rebuild = */ true);           /* the flows before this build are gone, whatever happens */
    if (t) *t = kmpgpu_timing{};
    if (n == 0) { c->flows_valid = true; return KMPGPU_OK; }
    HIP_TRY(hipSetDevice(c->device));
    hipError_t e = grow_buffer(&c->d_flow_table, &c->flow_table_cap, slots, EXACT);
    if (e == hipSuccess) e = grow_buffer(&c->d_flow_first, &c->flow_first_cap, slots, EXACT);
    if (e == hipSuccess) e = grow_buffer(&c->d_flow_of, &c->flow_of_cap, n, EIGHTH);
    if (e == hipSuccess) e = grow_buffer(&c->fr_ws, &c->fr_ws_cap, (uint64_t)kmp_extract_ws_bytes(n), EIGHTH);
    if (e == hipSuccess && !c->fr_tot) e = hipMalloc(&c->fr_tot, 2 * sizeof(unsigned long long));
    if (e != hipSuccess)
        return alloc_fail(e, "kmpgpu_flows_build: the table (%llu slots) and the ids (%llu payloads) could not be allocated", (unsigned long long)slots,
                          (unsigned long long)n);
    HIP_TRY(hipEventRecord(c->ev[0], c->stream));
    HIP_TRY(hipMemsetAsync(c->d_flow_table, 0, (size_t)slots * sizeof(uint32_t), c->stream));
    HIP_TRY(hipMemsetAsync(c->d_flow_first, 0xFF, (size_t)slots * sizeof(uint32_t), c->stream));
    HIP_TRY(profiled(c, [&] {
        return kmp_launch_flows_insert(c->d_meta, n, (flags & KMPGPU_FLOW_DIRECTED) != 0, c->d_flow_table, slots, c->d_flow_first, c->d_flow_of, c->stream);
    }));
    HIP_TRY(profiled(c, [&] { return kmp_launch_flows_firsts(c->d_flow_first, c->d_flow_of, n, c->fr_ws, c->stream); }));
    HIP_TRY(profiled(c, [&] { return kmp_launch_compact_scan(n, c->fr_ws, c->fr_tot, c->stream); }));
    HIP_TRY(hipMemcpyAsync(c->h_small, c->fr_tot, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));         /* (pinned: no staging) */
    HIP_TRY(hipStreamSynchronize(c->stream));
    unsigned long long tot[2] = {0, 0};
    memcpy(tot, c->h_small, sizeof tot);
    const uint64_t nf = tot[1];
    if (nf == 0 || nf > n) return fail(KMPGPU_EHIP, "kmpgpu_flows_build: %llu flows for %llu payloads", (unsigned long long)nf, (unsigned long long)n);
    e = grow_buffer(&c->d_flow_recs, &c->flow_recs_cap, nf, EIGHTH);
    if (e != hipSuccess) return alloc_fail(e, "kmpgpu_flows_build: the records (%llu flows) could not be allocated", (unsigned long long)nf);
    HIP_TRY(profiled(c, [&] { return kmp_launch_flows_number(c->d_meta, n, c->fr_ws, c->d_flow_of, c->d_flow_table, c->d_flow_recs, c->stream); }));
    HIP_TRY(profiled(c, [&] { return kmp_launch_flows_assign(c->d_flow_table, c->d_flow_of, c->d_len, n, c->d_flow_recs, c->stream); }));
    HIP_TRY(hipEventRecord(c->ev[1], c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (t) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
        t->kernel_ms = ms; t->launches = 6;
    }
    c->n_flows = nf; c->flows_valid = true;
    if (n_flows) *n_flows = nf;
    return KMPGPU_OK;
}

/* what kmpgpu_flows_read and kmpgpu_flow_ids_read share */
static int flows_read_range(kmpgpu_ctx *c, const char *who, void *out, const void *list, size_t size, uint64_t first, uint64_t n, uint64_t total)
{
    return read_range(c, who, c->flows_valid, "no flows (no kmpgpu_flows_build since the arena or its metadata were set)", out, list, size, first, n, total);
}

int kmpgpu_flows_read(kmpgpu_ctx *c, kmpgpu_flow *out, uint64_t first, uint64_t n)
{
    if (!c) return fail(KMPGPU_EINVAL, "kmpgpu_flows_read: ctx is NULL");
    return flows_read_range(c, "kmpgpu_flows_read", out, c->d_flow_recs, sizeof(kmpgpu_flow), first, n, c->n_flows);
}

int kmpgpu_flow_ids_read(kmpgpu_ctx *c, uint32_t *out, uint64_t first, uint64_t n)
{
    if (!c) return fail(KMPGPU_EINVAL, "kmpgpu_flow_ids_read: ctx is NULL");
    return flows_read_range(c, "kmpgpu_flow_ids_read", out, c->d_flow_of, sizeof(uint32_t), first, n, c->n_pkts);
}

/* The body of kmpgpu_scan_flows, and of kmpgpu_scan_flows_seams where sm is given: the context whose seam list (checked by the caller)
 * adds its pattern rows to the folded term rows. */
static int scan_flows_body(kmpgpu_ctx *c, const char *who, kmpgpu_ctx *sm, int family, uint32_t scope, uint64_t *flow_counts_out, uint64_t *any_out,
                           uint64_t *flow_hits_out, uint64_t *counts_out, kmpgpu_timing *t)
{
    if (!c) return fail(KMPGPU_EINVAL, "%s: ctx is NULL", who);
    if (family < KMPGPU_ALERT_PATTERNS || family > KMPGPU_ALERT_CHAINS) return fail(KMPGPU_EINVAL, "%s: family %d is none of KMPGPU_ALERT_*", who, family);
    if (scope != KMPGPU_FLOW_SCOPE_PACKET && scope != KMPGPU_FLOW_SCOPE_FLOW) return fail(KMPGPU_EINVAL, "%s: scope %u is none of KMPGPU_FLOW_SCOPE_*", who, scope);
    const bool per_flow = scope == KMPGPU_FLOW_SCOPE_FLOW;
    if (per_flow && family != KMPGPU_ALERT_RULES) return fail(KMPGPU_EINVAL, "%s: KMPGPU_FLOW_SCOPE_FLOW evaluates rules, family %d has none", who, family);
    if (!c->flows_valid) return fail(KMPGPU_ESTATE, "%s: no flows (no kmpgpu_flows_build since the arena or its metadata were set)", who);
    /* the rows of the family, as its own call checks them (no patterns for the patterns' own: the marking pass says so) */
    const uint64_t n_rows = family_n_rows(c, family);
    if (family != KMPGPU_ALERT_PATTERNS && (!c->d_patterns || c->n_pat == 0)) return fail(KMPGPU_ESTATE, "%s: no patterns set", who);
    if (family != KMPGPU_ALERT_PATTERNS && n_rows == 0)
        return fail(KMPGPU_ESTATE, "%s: no %s set", who, family == KMPGPU_ALERT_RULES ? "rules" : family == KMPGPU_ALERT_RELATIONS ? "relations" : "chains");
    if (c->fr_pending) return fail(KMPGPU_ESTATE, "%s: the context sits between kmpgpu_load_frames_begin and _finish", who);
    /* the seams first, on their own context's stream: the pass of kmpgpu_scan_packets, which runs beside src's where the streams differ.
     * Its any[] lets the fold skip the words no pattern has a bit in.  An empty list (a context without an arena) adds nothing */
    MarkPass ps;
    FamilyRows fs;
    bool seams = false;
    if (sm && c->n_pkts) {
        const int rs = begin_family(sm, who, KMPGPU_ALERT_PATTERNS, nullptr, nullptr, nullptr, &ps);
        if (rs) return rs;
        seams = !ps.empty;
        if (seams) {
            const int re = enqueue_family(sm, who, KMPGPU_ALERT_PATTERNS, ps, /* profile_reduce = */ false, &fs);
            if (re) return re;
            HIP_TRY(hipSetDevice(c->device));
        }
    }
    MarkPass p;
    const int rc = begin_family(c, who, family, flow_counts_out, counts_out, t, &p);
    if (rc || p.empty) return rc;
    FamilyRows f;
    const int rr = enqueue_family(c, who, family, p, /* profile_reduce = */ true, &f);
    if (rr) return rr;
    /* the folded matrix, rows of an even number of words as the reduce and the rules kernel read them: SCOPE_PACKET [family's rows x Sf]
     * [flow_counts rows][any Sf]; SCOPE_FLOW [term rows x Sf][rule rows x Sf][flow_counts rules][any Sf] */
    const uint64_t Wf = (c->n_flows + 63u) / 64u, Sf = (Wf + 1u) & ~1ull;
    const uint64_t n_terms = (uint64_t)c->n_pat + c->n_rel + c->n_chains + c->n_hdr + c->n_bt + c->n_rx + c->n_links;
    const uint64_t fold_rows = per_flow ? n_terms : n_rows, out_rows = per_flow ? n_terms + n_rows : n_rows;
    const uint64_t words = out_rows * Sf + n_rows + Sf;
    const hipError_t e = grow_buffer(&c->d_flow_fold, &c->flow_fold_cap, words, EIGHTH);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(c->stream);      /* the pass is under way on the stream; the context stays usable */
        return alloc_fail(e, "%s: the folded matrix (%llu bytes) could not be allocated", who, (unsigned long long)(words * 8u));
    }
    unsigned long long *d_rows = c->d_flow_fold + (per_flow ? n_terms * Sf : 0), *d_fc = c->d_flow_fold + out_rows * Sf, *d_any = d_fc + n_rows;
    HIP_TRY(hipMemsetAsync(c->d_flow_fold, 0, (size_t)words * sizeof(unsigned long long), c->stream));
    hipEvent_t e1;
    HIP_TRY(profile_launch(c, &e1));
    /* SCOPE_FLOW folds the whole hit matrix, and no any[] covers all of its rows */
    HIP_TRY(kmp_launch_flows_fold(per_flow ? p.d_mat : f.d_rows, p.stride, (uint32_t)fold_rows, c->n_pkts, per_flow ? nullptr : f.d_any, c->d_flow_of,
                                  c->n_flows, c->d_flow_fold, Sf, c->stream));
    HIP_TRY(profile_launched(c, e1));
    if (seams) {
        /* the same kernel a second time: its output is an atomic OR into the matrix zeroed above */
        HIP_TRY(hipStreamSynchronize(sm->stream));                  /* the seams' pass has landed in its matrix */
        HIP_TRY(profiled(c, [&] {
            return kmp_launch_flows_fold(ps.d_mat, ps.stride, c->n_pat, sm->n_pkts, fs.d_any, sm->d_seam_flow, c->n_flows, c->d_flow_fold, Sf, c->stream);
        }));
    }
    HIP_TRY(profile_launch(c, &e1));
    if (per_flow)
        HIP_TRY(kmp_launch_rules(c->d_flow_fold, Sf, c->n_flows, c->d_rule_heads, c->d_rule_quads, c->n_rules, d_rows, d_fc, d_any, c->stream));
    else
        HIP_TRY(kmp_launch_marks_reduce(d_rows, (uint32_t)n_rows, Sf, d_fc, d_any, c->stream));
    HIP_TRY(profile_launched(c, e1));
    HIP_TRY(hipEventRecord(c->ev[1], c->stream));
    if (flow_counts_out) HIP_TRY(hipMemcpyAsync(flow_counts_out, d_fc, (size_t)n_rows * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    if (any_out) HIP_TRY(hipMemcpyAsync(any_out, d_any, Wf * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    if (counts_out) HIP_TRY(hipMemcpyAsync(counts_out, p.d_cnt, (size_t)c->n_pat * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    if (flow_hits_out) HIP_TRY(download_rows(c, flow_hits_out, d_rows, Wf, Sf, n_rows));
    return finish_marking(c, p.launches + f.launches + 2u + (seams ? ps.launches + fs.launches + 1u : 0u), t);
}

int kmpgpu_scan_flows(kmpgpu_ctx *c, int family, uint32_t scope, uint64_t *flow_counts_out, uint64_t *any_out, uint64_t *flow_hits_out,
                      uint64_t *counts_out, kmpgpu_timing *t)
{
    return scan_flows_body(c, "kmpgpu_scan_flows", nullptr, family, scope, flow_counts_out, any_out, flow_hits_out, counts_out, t);
}

int kmpgpu_scan_flows_seams(kmpgpu_ctx *c, kmpgpu_ctx *sm, uint64_t *flow_counts_out, uint64_t *any_out, uint64_t *flow_hits_out, uint64_t *counts_out,
                            kmpgpu_timing *t)
{
    const char *who = "kmpgpu_scan_flows_seams";
    if (!c || !sm) return fail(KMPGPU_EINVAL, "%s: ctx is NULL", who);
    if (c == sm) return fail(KMPGPU_EINVAL, "%s: src and seams are the same context", who);
    if (c->device != sm->device) return fail(KMPGPU_EINVAL, "%s: the contexts sit on devices %d and %d", who, c->device, sm->device);
    if (!c->flows_valid) return fail(KMPGPU_ESTATE, "%s: no flows (no kmpgpu_flows_build since the arena or its metadata were set)", who);
    if (sm->fr_pending) return fail(KMPGPU_ESTATE, "%s: seams sits between kmpgpu_load_frames_begin and _finish", who);
    if (!sm->seams_valid) return fail(KMPGPU_ESTATE, "%s: no seams (no kmpgpu_load_seams since the arena was set)", who);
    if (sm->seam_src != c->id || sm->seam_gen != c->flows_gen)
        return fail(KMPGPU_ESTATE, "%s: the seam list was not built from src's current flows", who);
    if (c->n_pat != sm->n_pat || c->pat_sig != sm->pat_sig) return fail(KMPGPU_ESTATE, "%s: the contexts do not hold the same patterns", who);
    return scan_flows_body(c, who, sm, KMPGPU_ALERT_RULES, KMPGPU_FLOW_SCOPE_FLOW, flow_counts_out, any_out, flow_hits_out, counts_out, t);
}

int kmpgpu_set_flowbits(kmpgpu_ctx *c, const kmpgpu_flowbit_op *ops, uint32_t n_ops, uint32_t n_bits)
{
    const int sr = setter_state(c, "kmpgpu_set_flowbits");
    if (sr) return sr;
    if (c->n_rules == 0) return fail(KMPGPU_ESTATE, "kmpgpu_set_flowbits: no rules set");
    kmp_flowbit_tables tb;
    std::string msg;
    if (n_ops) {
        const int rc = kmp_pack_flowbits(ops, n_ops, n_bits, c->n_rules, &tb, &msg);
        if (rc) return fail(rc, "%s", msg.c_str());
        if (tb.acting.empty()) tb.acting.assign(8, 0u);          /* tests only: one record nobody reads, never a NULL table */
    }
    const int rc = swap_tables(c, "kmpgpu_set_flowbits: the ops", {{tb.acting, (void **)&c->d_fb_acting}, {tb.tests, (void **)&c->d_fb_tests}});
    if (rc) return rc;
    c->n_fb_bits = tb.n_bits;
    c->fb_level_mask = tb.level_mask;
    c->fb_level_first = tb.level_first;
    return KMPGPU_OK;
}

int kmpgpu_scan_flowbits(kmpgpu_ctx *c, uint64_t *rule_pkt_counts_out, uint64_t *any_out, uint64_t *rule_hits_out, uint64_t *state_out,
                         uint32_t *flow_state_out, uint64_t *counts_out, kmpgpu_timing *t)
{
    const char *who = "kmpgpu_scan_flowbits";
    if (!c) return fail(KMPGPU_EINVAL, "%s: ctx is NULL", who);
    if (c->n_rules == 0) return fail(KMPGPU_ESTATE, "%s: no rules set", who);
    if (c->n_fb_bits == 0) return fail(KMPGPU_ESTATE, "%s: no flow bits (kmpgpu_set_flowbits)", who);
    if (!c->flows_valid) return fail(KMPGPU_ESTATE, "%s: no flows (no kmpgpu_flows_build since the arena or its metadata were set)", who);
    if (c->fr_pending) return fail(KMPGPU_ESTATE, "%s: the context sits between kmpgpu_load_frames_begin and _finish", who);
    MarkPass p;
    const int rc = begin_family(c, who, KMPGPU_ALERT_RULES, rule_pkt_counts_out, counts_out, t, &p);
    if (rc || p.empty) return rc;
    FamilyRows f;
    const int rr = enqueue_family(c, who, KMPGPU_ALERT_RULES, p, /* profile_reduce = */ false, &f);
    if (rr) return rr;
    uint32_t launches = p.launches + f.launches;
    const uint64_t n = c->n_pkts, nf = c->n_flows, nb = c->n_fb_bits, nr = c->n_rules;
    /* the order is the flows': built once per generation */
    const bool ordered = c->fb_order_valid && c->fb_order_gen == c->flows_gen;
    const uint64_t order_bytes = ordered ? c->fb_order_cap : (uint64_t)kmp_flowbits_order_bytes(n, nf);
    const uint64_t scan_bytes = (uint64_t)kmp_flowbits_ws_bytes(n), ws_bytes = scan_bytes + 4u * (n + nf);
    const uint64_t out_words = (nb + nr) * p.stride + nr + p.stride;
    hipError_t e = order_bytes ? hipSuccess : hipErrorInvalidValue;               /* (0: rocPRIM refused the size query) */
    if (e == hipSuccess && !ordered) { c->fb_order_valid = false; e = grow_buffer(&c->d_fb_order, &c->fb_order_cap, order_bytes, EIGHTH); }
    if (e == hipSuccess) e = grow_buffer(&c->d_fb_ws, &c->fb_ws_cap, ws_bytes, EIGHTH);
    if (e == hipSuccess) e = grow_buffer(&c->d_fb_out, &c->fb_out_cap, out_words, EIGHTH);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(c->stream);      /* the pass is under way on the stream; the context stays usable */
        return alloc_fail(e, "%s: the order, the scan workspace and the rows (%llu bytes) could not be allocated", who,
                          (unsigned long long)(order_bytes + ws_bytes + out_words * 8u));
    }
    uint32_t *d_before32 = reinterpret_cast<uint32_t *>(c->d_fb_ws + scan_bytes), *d_flow_state = d_before32 + n;
    unsigned long long *d_before = c->d_fb_out, *d_alert = d_before + nb * p.stride, *d_pc = d_alert + nr * p.stride, *d_any = d_pc + nr;
    HIP_TRY(hipMemsetAsync(d_before32, 0, (size_t)(4u * (n + nf)), c->stream));
    HIP_TRY(hipMemsetAsync(c->d_fb_out, 0, (size_t)out_words * sizeof(unsigned long long), c->stream));
    if (!ordered) {
        HIP_TRY(profiled(c, [&] { return kmp_launch_flowbits_order(c->d_flow_of, n, nf, c->d_fb_order, (size_t)c->fb_order_cap, c->stream); }));
        c->fb_order_valid = true; c->fb_order_gen = c->flows_gen;
        launches += 2u;
    }
    for (size_t l = 0; l < c->fb_level_mask.size(); l++) {
        const uint32_t first = c->fb_level_first[l], n_act = c->fb_level_first[l + 1] - first;
        if (n_act == 0) continue;                   /* bits that are tested only: 0 for ever */
        HIP_TRY(profiled(c, [&] {
            return kmp_launch_flowbits_build(f.d_rows, p.stride, n, c->d_fb_acting + 2u * (size_t)first, n_act, d_before32, c->d_fb_order, c->d_fb_ws, c->stream);
        }));
        HIP_TRY(profiled(c, [&] { return kmp_launch_flowbits_scan(n, c->d_flow_of, c->d_fb_order, c->d_fb_ws, d_before32, d_flow_state, &launches, c->stream); }));
        HIP_TRY(profiled(c, [&] { return kmp_launch_flowbits_rows(d_before32, n, c->fb_level_mask[l], p.stride, d_before, c->stream); }));
        launches += 2u;
    }
    HIP_TRY(profiled(c, [&] { return kmp_launch_flowbits_final(f.d_rows, d_before, p.stride, c->d_fb_tests, c->n_rules, d_alert, d_pc, d_any, c->stream); }));
    launches++;
    HIP_TRY(hipEventRecord(c->ev[1], c->stream));
    if (rule_pkt_counts_out) HIP_TRY(hipMemcpyAsync(rule_pkt_counts_out, d_pc, (size_t)nr * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    if (any_out) HIP_TRY(hipMemcpyAsync(any_out, d_any, p.W * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    if (counts_out) HIP_TRY(hipMemcpyAsync(counts_out, p.d_cnt, (size_t)c->n_pat * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    if (rule_hits_out) HIP_TRY(download_rows(c, rule_hits_out, d_alert, p.W, p.stride, nr));
    if (state_out) HIP_TRY(download_rows(c, state_out, d_before, p.W, p.stride, nb));
    if (flow_state_out) HIP_TRY(hipMemcpyAsync(flow_state_out, d_flow_state, (size_t)nf * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    return finish_marking(c, launches, t);
}

int kmpgpu_set_thresholds(kmpgpu_ctx *c, const kmpgpu_threshold *thr, uint32_t n_thr)
{
    static_assert(sizeof(kmpgpu_threshold) == 24, "kmpgpu_threshold is the 24-byte record of kmpgpu.h");
    const int sr = setter_state(c, "kmpgpu_set_thresholds");
    if (sr) return sr;
    if (c->n_rules == 0) return fail(KMPGPU_ESTATE, "kmpgpu_set_thresholds: no rules set");
    kmp_threshold_tables tb;
    std::string msg;
    if (n_thr) {
        const int rc = kmp_pack_thresholds(thr, n_thr, c->n_rules, &tb, &msg);
        if (rc) return fail(rc, "%s", msg.c_str());
    }
    const int rc = swap_tables(c, "kmpgpu_set_thresholds: the thresholds", {{tb.final_table, (void **)&c->d_thr_table}});
    if (rc) return rc;
    c->thr.assign(thr, thr + n_thr);
    for (int x = 0; x < 4; x++) c->thr_by_track[x] = tb.by_track[x];
    c->thr_windowed = tb.windowed;
    return KMPGPU_OK;
}

int kmpgpu_scan_thresholds(kmpgpu_ctx *c, const uint64_t *ts, int ts_on_device, uint64_t *rule_pkt_counts_out, uint64_t *any_out,
                           uint64_t *rule_hits_out, uint32_t *window_counts_out, uint64_t *counts_out, kmpgpu_timing *t)
{
    const char *who = "kmpgpu_scan_thresholds";
    if (!c) return fail(KMPGPU_EINVAL, "%s: ctx is NULL", who);
    if (ts_on_device != 0 && ts_on_device != 1) return fail(KMPGPU_EINVAL, "%s: ts_on_device is %d, not 0 or 1", who, ts_on_device);
    if (c->n_rules == 0) return fail(KMPGPU_ESTATE, "%s: no rules set", who);
    if (c->thr.empty()) return fail(KMPGPU_ESTATE, "%s: no thresholds (kmpgpu_set_thresholds)", who);
    if (!c->arena_seen) return fail(KMPGPU_ESTATE, "%s: no arena loaded", who);
    if (c->fr_pending) return fail(KMPGPU_ESTATE, "%s: the context sits between kmpgpu_load_frames_begin and _finish", who);
    const bool by_addr[2] = {!c->thr_by_track[KMPGPU_THR_BY_SRC].empty(), !c->thr_by_track[KMPGPU_THR_BY_DST].empty()};
    const bool by_flow = !c->thr_by_track[KMPGPU_THR_BY_FLOW].empty();
    if ((by_addr[0] || by_addr[1]) && c->n_pkts && !c->has_meta)
        return fail(KMPGPU_ESTATE, "%s: no packet metadata (KMPGPU_OPT_KEEP_META, kmpgpu_set_meta)", who);
    if (by_flow && !c->flows_valid) return fail(KMPGPU_ESTATE, "%s: no flows (no kmpgpu_flows_build since the arena or its metadata were set)", who);
    if (!ts && c->n_pkts) return fail(KMPGPU_EINVAL, "%s: ts is NULL", who);
    if (ts_on_device && ((uintptr_t)ts & 7u)) return fail(KMPGPU_EINVAL, "%s: the device timestamps are not 8-byte aligned", who);
    MarkPass p;
    const int rc = begin_family(c, who, KMPGPU_ALERT_RULES, rule_pkt_counts_out, counts_out, t, &p);
    if (rc || p.empty) return rc;
    FamilyRows f;
    const int rr = enqueue_family(c, who, KMPGPU_ALERT_RULES, p, /* profile_reduce = */ false, &f);
    if (rr) return rr;
    uint32_t launches = p.launches + f.launches;
    const uint64_t n = c->n_pkts, nr = c->n_rules, nq = c->thr.size(), P = kmp_thresholds_pad(n);
    /* the orders in use: [0] by source, [1] by destination (this call's own, per generation of the metadata), [2] the flows' (kmpgpu_scan_flowbits') */
    const bool ordered[3] = {c->thr_order_valid[0] && c->thr_order_gen[0] == c->meta_gen, c->thr_order_valid[1] && c->thr_order_gen[1] == c->meta_gen,
                             c->fb_order_valid && c->fb_order_gen == c->flows_gen};
    const bool used[3] = {by_addr[0], by_addr[1], by_flow};
    uint8_t **order_buf[3] = {&c->d_thr_order[0], &c->d_thr_order[1], &c->d_fb_order};
    uint64_t *order_cap[3] = {&c->thr_order_cap[0], &c->thr_order_cap[1], &c->fb_order_cap};
    /* the workspace: T, the aggregates, T in the order of every sorted track in use, the prefix sum (before it: the addresses to sort) */
    const uint64_t agg_bytes = (uint64_t)kmp_thresholds_agg_bytes(n);
    uint64_t ws_bytes = 8u * P + agg_bytes + 4u * P, out_words = (nq + nr) * p.stride + nr + p.stride;
    for (int x = 0; x < 3; x++) if (used[x] && c->thr_windowed) ws_bytes += 8u * P;
    hipError_t e = hipSuccess;
    for (int x = 0; x < 3 && e == hipSuccess; x++) {
        if (!used[x] || ordered[x]) continue;
        const uint64_t bytes = (uint64_t)kmp_flowbits_order_bytes(n, x == 2 ? c->n_flows : 1ull << 32);
        if (!bytes) { e = hipErrorInvalidValue; break; }                          /* (rocPRIM refused the size query) */
        if (x == 2) c->fb_order_valid = false; else c->thr_order_valid[x] = false;
        e = grow_buffer(order_buf[x], order_cap[x], bytes, EIGHTH);
    }
    if (e == hipSuccess) e = grow_buffer(&c->d_thr_ws, &c->thr_ws_cap, ws_bytes, EIGHTH);
    if (e == hipSuccess) e = grow_buffer(&c->d_thr_out, &c->thr_out_cap, out_words, EIGHTH);
    if (e == hipSuccess && window_counts_out) e = grow_buffer(&c->d_thr_wc, &c->thr_wc_cap, nq * n, EIGHTH);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(c->stream);      /* the pass is under way on the stream; the context stays usable */
        return alloc_fail(e, "%s: the orders, the scans' workspace (%llu bytes) and the rows (%llu bytes) could not be allocated", who,
                          (unsigned long long)ws_bytes, (unsigned long long)(out_words * 8u));
    }
    unsigned long long *d_T = reinterpret_cast<unsigned long long *>(c->d_thr_ws), *d_Ts[3] = {nullptr, nullptr, nullptr};
    uint8_t *d_agg = c->d_thr_ws + 8u * P, *at = d_agg + agg_bytes;
    for (int x = 0; x < 3; x++) if (used[x] && c->thr_windowed) { d_Ts[x] = reinterpret_cast<unsigned long long *>(at); at += 8u * P; }
    uint32_t *d_C = reinterpret_cast<uint32_t *>(at);
    unsigned long long *d_pass = c->d_thr_out, *d_alert = d_pass + nq * p.stride, *d_pc = d_alert + nr * p.stride, *d_any = d_pc + nr;
    HIP_TRY(hipMemsetAsync(c->d_thr_out, 0, (size_t)out_words * sizeof(unsigned long long), c->stream));
    hipEvent_t e1;
    if (c->thr_windowed) {
        if (ts_on_device) HIP_TRY(hipMemcpyAsync(d_T, ts, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToDevice, c->stream));
        else HIP_TRY(upload_split(d_T, reinterpret_cast<const uint8_t *>(ts), n * sizeof(uint64_t), c->stream));
        HIP_TRY(profiled(c, [&] { return kmp_launch_thresholds_time(d_T, n, d_agg, &launches, c->stream); }));
    }
    for (int x = 0; x < 3; x++) {
        if (!used[x]) continue;
        if (!ordered[x]) {
            HIP_TRY(profile_launch(c, &e1));
            if (x < 2) {
                HIP_TRY(kmp_launch_thresholds_keys(c->d_meta, n, x == 1, d_C, c->stream));
                launches++;
            }
            HIP_TRY(kmp_launch_flowbits_order(x == 2 ? c->d_flow_of : d_C, n, x == 2 ? c->n_flows : 1ull << 32, *order_buf[x], (size_t)*order_cap[x], c->stream));
            HIP_TRY(profile_launched(c, e1));
            if (x == 2) { c->fb_order_valid = true; c->fb_order_gen = c->flows_gen; }
            else { c->thr_order_valid[x] = true; c->thr_order_gen[x] = c->meta_gen; }
            launches += 2u;
        }
        if (d_Ts[x]) {
            HIP_TRY(profiled(c, [&] { return kmp_launch_thresholds_tsort(d_T, *order_buf[x], n, d_Ts[x], c->stream); }));
            launches++;
        }
    }
    for (int track = 0; track < 4; track++) {
        const uint8_t *ob = track == KMPGPU_THR_BY_RULE ? nullptr : *order_buf[track - 1];
        const unsigned long long *Ts = track == KMPGPU_THR_BY_RULE ? (c->thr_windowed ? d_T : nullptr) : d_Ts[track - 1];
        for (const uint32_t q : c->thr_by_track[track]) {
            const kmpgpu_threshold &th = c->thr[q];
            const unsigned long long *row = f.d_rows + (uint64_t)th.rule * p.stride;
            HIP_TRY(profiled(c, [&] { return kmp_launch_thresholds_count(row, n, ob, d_C, d_agg, &launches, c->stream); }));
            HIP_TRY(profiled(c, [&] {
                return kmp_launch_thresholds_pass(row, n, ob, Ts, d_C, th.type, th.count, th.window, d_pass + (uint64_t)q * p.stride,
                                                  window_counts_out ? c->d_thr_wc + (uint64_t)q * n : nullptr, c->stream);
            }));
            launches++;
        }
    }
    HIP_TRY(profiled(c, [&] { return kmp_launch_thresholds_final(f.d_rows, d_pass, p.stride, c->d_thr_table, c->n_rules, d_alert, d_pc, d_any, c->stream); }));
    launches++;
    HIP_TRY(hipEventRecord(c->ev[1], c->stream));
    if (rule_pkt_counts_out) HIP_TRY(hipMemcpyAsync(rule_pkt_counts_out, d_pc, (size_t)nr * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    if (any_out) HIP_TRY(hipMemcpyAsync(any_out, d_any, p.W * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    if (counts_out) HIP_TRY(hipMemcpyAsync(counts_out, p.d_cnt, (size_t)c->n_pat * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    if (rule_hits_out) HIP_TRY(download_rows(c, rule_hits_out, d_alert, p.W, p.stride, nr));
    if (window_counts_out) HIP_TRY(hipMemcpyAsync(window_counts_out, c->d_thr_wc, (size_t)(nq * n) * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    return finish_marking(c, launches, t);
}

int kmpgpu_flows_select(kmpgpu_ctx *c, const void *flow_bits, int on_device, uint64_t *pkt_bits_out, const void **d_pkt_bits)
{
    if (!c) return fail(KMPGPU_EINVAL, "kmpgpu_flows_select: ctx is NULL");
    if (d_pkt_bits) *d_pkt_bits = nullptr;
    if (on_device != 0 && on_device != 1) return fail(KMPGPU_EINVAL, "kmpgpu_flows_select: on_device is %d, not 0 or 1", on_device);
    if (!c->flows_valid) return fail(KMPGPU_ESTATE, "kmpgpu_flows_select: no flows (no kmpgpu_flows_build since the arena or its metadata were set)");
    if (c->n_pkts == 0) return KMPGPU_OK;
    if (!flow_bits) return fail(KMPGPU_EINVAL, "kmpgpu_flows_select: flow_bits is NULL");
    if (on_device && ((uintptr_t)flow_bits & 7u)) return fail(KMPGPU_EINVAL, "kmpgpu_flows_select: the device bitmap is not 8-byte aligned");
    HIP_TRY(hipSetDevice(c->device));
    const uint64_t W = (c->n_pkts + 63u) / 64u, Wf = (c->n_flows + 63u) / 64u;
    HIP_TRY(hipStreamSynchronize(c->stream));      /* the bitmap of the select before this one may still be read */
    const hipError_t e = grow_buffer(&c->d_flow_sel, &c->flow_sel_cap, W + Wf, EIGHTH);
    if (e != hipSuccess) return alloc_fail(e, "kmpgpu_flows_select: the bitmaps (%llu bytes) could not be allocated", (unsigned long long)((W + Wf) * 8u));
    const unsigned long long *d_bits = (const unsigned long long *)flow_bits;
    if (!on_device) {
        HIP_TRY(hipMemcpyAsync(c->d_flow_sel + W, flow_bits, Wf * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
        d_bits = c->d_flow_sel + W;
    }
    HIP_TRY(kmp_launch_flows_expand(d_bits, c->d_flow_of, c->n_pkts, c->d_flow_sel, c->stream));
    if (pkt_bits_out) HIP_TRY(hipMemcpyAsync(pkt_bits_out, c->d_flow_sel, W * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (d_pkt_bits) *d_pkt_bits = c->d_flow_sel;
    return KMPGPU_OK;
}

int kmpgpu_synth_fill(kmpgpu_ctx *c, void *d_arena, const void *d_pkt_off, const void *d_pkt_len, uint64_t first_pkt_id,
                      uint64_t n_pkts, const kmp_synth_params *sp)
{
    if (!c || !sp) return fail(KMPGPU_EINVAL, "kmpgpu_synth_fill: NULL argument");
    if (n_pkts && (!d_arena || !d_pkt_off || !d_pkt_len)) return fail(KMPGPU_EINVAL, "kmpgpu_synth_fill: NULL buffers");
    if (sp->needle_len > KMP_SYNTH_MAX_NEEDLE || sp->span == 0 || sp->span > 256 || sp->lo + sp->span > 256)
        return fail(KMPGPU_EINVAL, "kmpgpu_synth_fill: bad generator parameters");
    HIP_TRY(hipSetDevice(c->device));
    if (d_arena == (const void *)c->d_arena) c->fold_stale = true;
    HIP_TRY(kmp_launch_synth_fill((uint8_t *)d_arena, (const uint64_t *)d_pkt_off, (const uint32_t *)d_pkt_len, first_pkt_id,
                                  n_pkts, *sp, c->stream));
    return KMPGPU_OK;
}

int kmpgpu_fixed_index(kmpgpu_ctx *c, void *d_pkt_off, void *d_pkt_len, uint64_t n_pkts, uint32_t len, uint32_t slot_align)
{
    if (!c) return fail(KMPGPU_EINVAL, "kmpgpu_fixed_index: ctx is NULL");
    if (slot_align < 16 || (slot_align & (slot_align - 1))) return fail(KMPGPU_EINVAL, "slot_align must be a power of two >= 16");
    HIP_TRY(hipSetDevice(c->device));
    const uint64_t stride = ((uint64_t)len + slot_align - 1) & ~((uint64_t)slot_align - 1);
    HIP_TRY(kmp_launch_fixed_index((uint64_t *)d_pkt_off, (uint32_t *)d_pkt_len, n_pkts, len, stride ? stride : slot_align, c->stream));
    return KMPGPU_OK;
}

int kmpgpu_arena_info(kmpgpu_ctx *c, uint64_t *n_pkts, uint64_t *payload_bytes)
{
    if (!c) return fail(KMPGPU_EINVAL, "kmpgpu_arena_info: ctx is NULL");
    if (n_pkts) *n_pkts = c->n_pkts;
    if (payload_bytes) *payload_bytes = c->payload_bytes;
    return KMPGPU_OK;
}

int kmpgpu_effective_bytes(kmpgpu_ctx *c, uint64_t *bytes_out)
{
    if (!c || !bytes_out) return fail(KMPGPU_EINVAL, "kmpgpu_effective_bytes: NULL argument");
    *bytes_out = 0;
    if (c->n_pkts == 0) return KMPGPU_OK;
    HIP_TRY(hipSetDevice(c->device));
    unsigned long long *d = nullptr, h = 0ull;
    HIP_TRY(hipMalloc(&d, sizeof h));
    hipError_t e = hipMemsetAsync(d, 0, sizeof h, c->stream);
    if (e == hipSuccess) e = kmp_launch_effective_bytes(c->d_arena, c->d_off, c->d_len, c->n_pkts, d, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&h, d, sizeof h, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(KMPGPU_EHIP, "kmpgpu_effective_bytes: %s", hipGetErrorString(e));
    *bytes_out = h;
    return KMPGPU_OK;
}

int kmpgpu_arena_download(kmpgpu_ctx *c, uint8_t *arena_out, uint64_t arena_cap, uint64_t *arena_bytes, uint64_t *pkt_off_out,
                          uint32_t *pkt_len_out)
{
    if (!c) return fail(KMPGPU_EINVAL, "kmpgpu_arena_download: ctx is NULL");
    if (arena_bytes) *arena_bytes = c->arena_bytes;
    if (c->n_pkts == 0) return KMPGPU_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (arena_out) {
        if (arena_cap < c->arena_bytes) return fail(KMPGPU_EINVAL, "kmpgpu_arena_download: buffer too small");
        HIP_TRY(hipMemcpy(arena_out, c->d_arena, c->arena_bytes, hipMemcpyDeviceToHost));
    }
    if (pkt_off_out) HIP_TRY(hipMemcpy(pkt_off_out, c->d_off, c->n_pkts * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (pkt_len_out) HIP_TRY(hipMemcpy(pkt_len_out, c->d_len, c->n_pkts * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return KMPGPU_OK;
}

}  // extern "C"

/* ---- RCCL count reduce (mpi_dumping.c:202) -------------------------------------------------------------- */
namespace {
struct RcclApi {
    void *handle = nullptr;
    ncclResult_t (*CommInitAll)(ncclComm_t *, int, const int *) = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
};
RcclApi g_rccl;

int rccl_load()
{
    static std::mutex mu;           /* contexts are per thread (bin/openmp_data brings its shards up on threads); the library handle is not */
    std::lock_guard<std::mutex> lock(mu);
    static int state = 0;           /* 0 untried, 1 loaded, -1 failed */
    if (state == 1) return KMPGPU_OK;
    if (state == -1) return fail(KMPGPU_EHIP, "librccl.so could not be loaded");
    /* RCCL writes its version banner and NCCL_DEBUG output to stdout unless told otherwise; stdout belongs to the
     * caller (the drop-in programs' report, serial.c:163-169, is compared byte for byte) */
    setenv("NCCL_DEBUG_FILE", "/dev/stderr", 0);
    void *h = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
    if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!h) { state = -1; return fail(KMPGPU_EHIP, "cannot load librccl.so: %s", dlerror()); }
    g_rccl.handle = h;
#define KMP_RCCL_SYM(field, name) do { *(void **)(&g_rccl.field) = dlsym(h, name); \
        if (!g_rccl.field) { state = -1; return fail(KMPGPU_EHIP, "librccl.so lacks %s", name); } } while (0)
    KMP_RCCL_SYM(CommInitAll, "ncclCommInitAll");
    KMP_RCCL_SYM(GetUniqueId, "ncclGetUniqueId");
    KMP_RCCL_SYM(CommInitRank, "ncclCommInitRank");
    KMP_RCCL_SYM(AllReduce, "ncclAllReduce");
    KMP_RCCL_SYM(GroupStart, "ncclGroupStart");
    KMP_RCCL_SYM(GroupEnd, "ncclGroupEnd");
    KMP_RCCL_SYM(CommDestroy, "ncclCommDestroy");
    KMP_RCCL_SYM(GetErrorString, "ncclGetErrorString");
#undef KMP_RCCL_SYM
    state = 1;
    return KMPGPU_OK;
}
/* RCCL prints its version banner (NCCL_DEBUG=VERSION and above) with printf on the first communicator: stdout belongs
 * to the caller -- the drop-in programs' report (serial.c:163-169) is compared byte for byte -- so file descriptor 1
 * points at stderr while a communicator is being created.  Guards may overlap (one thread per GPU inside
 * kmpgpu_comm_init_rank, which blocks until every rank has joined): the first one in saves and redirects, the last one
 * out restores, under a mutex.  (Another thread of the caller that writes to stdout in exactly that window lands on
 * stderr too.) */
struct StdoutToStderr {
    static std::mutex &mu() { static std::mutex m; return m; }
    static int &depth() { static int d = 0; return d; }
    static int &saved() { static int fd = -1; return fd; }
    StdoutToStderr()
    {
        std::lock_guard<std::mutex> lock(mu());
        if (depth()++ != 0) return;
        fflush(stdout);
        saved() = dup(1);
        if (saved() >= 0 && dup2(2, 1) < 0) { close(saved()); saved() = -1; }
    }
    ~StdoutToStderr()
    {
        std::lock_guard<std::mutex> lock(mu());
        if (--depth() != 0 || saved() < 0) return;
        fflush(stdout);
        (void)dup2(saved(), 1);
        close(saved());
        saved() = -1;
    }
};
#define RCCL_TRY(expr)                                                                                        \
    do {                                                                                                    \
        ncclResult_t r_ = (expr);                                                                           \
        if (r_ != ncclSuccess) return fail(KMPGPU_EHIP, "%s failed: %s", #expr, g_rccl.GetErrorString(r_)); \
    } while (0)
}  // namespace

struct kmpgpu_comm {
    std::vector<kmpgpu_ctx *> ctx;          /* the local ranks' contexts (nullptr: destroyed before the communicator) */
    std::vector<ncclComm_t>   comm;         /* one communicator handle per local rank */
    std::vector<int>          device;       /* copies: kmpgpu_comm_destroy must not need the contexts */
    int n_ranks = 0;
};

static void comm_forget(kmpgpu_comm *k, kmpgpu_ctx *c)
{
    for (size_t i = 0; i < k->ctx.size(); i++)
        if (k->ctx[i] == c) {
            /* the rank's collectives were enqueued on the context's stream, which is about to go: let them finish */
            (void)hipSetDevice(c->device);
            if (c->stream) (void)hipStreamSynchronize(c->stream);
            k->ctx[i] = nullptr;
        }
    c->comm = nullptr;
}

extern "C" {

int kmpgpu_device_of(kmpgpu_ctx *c) { return c ? c->device : fail(KMPGPU_EINVAL, "kmpgpu_device_of: ctx is NULL"); }

int kmpgpu_comm_init(kmpgpu_comm **out, kmpgpu_ctx *const *ctx, int n_ctx)
{
    if (!out || !ctx || n_ctx < 1) return fail(KMPGPU_EINVAL, "kmpgpu_comm_init: bad arguments");
    *out = nullptr;
    std::vector<int> devs;
    for (int i = 0; i < n_ctx; i++) {
        if (!ctx[i]) return fail(KMPGPU_EINVAL, "kmpgpu_comm_init: context %d is NULL", i);
        if (ctx[i]->comm) return fail(KMPGPU_EINVAL, "kmpgpu_comm_init: context %d already belongs to a communicator", i);
        if (ctx[i]->n_pat != ctx[0]->n_pat) return fail(KMPGPU_EINVAL, "kmpgpu_comm_init: context %d holds %u patterns, context 0 %u", i, ctx[i]->n_pat, ctx[0]->n_pat);
        for (int d : devs)
            if (d == ctx[i]->device)
                return fail(KMPGPU_EINVAL, "kmpgpu_comm_init: two contexts on device %d (one rank per device: sum the counts of contexts that share a GPU on the host)", d);
        devs.push_back(ctx[i]->device);
    }
    int rc = rccl_load();
    if (rc) return rc;
    kmpgpu_comm *k = new (std::nothrow) kmpgpu_comm();
    if (!k) return fail(KMPGPU_ENOMEM, "kmpgpu_comm_init: out of host memory");
    k->ctx.assign(ctx, ctx + n_ctx);
    k->comm.assign((size_t)n_ctx, nullptr);
    k->n_ranks = n_ctx;
    ncclResult_t r;
    { StdoutToStderr guard; r = g_rccl.CommInitAll(k->comm.data(), n_ctx, devs.data()); }
    if (r != ncclSuccess) { delete k; return fail(KMPGPU_EHIP, "ncclCommInitAll failed: %s", g_rccl.GetErrorString(r)); }
    k->device = devs;
    for (int i = 0; i < n_ctx; i++) ctx[i]->comm = k;
    *out = k;
    return KMPGPU_OK;
}

int kmpgpu_comm_unique_id(void *id_out)
{
    if (!id_out) return fail(KMPGPU_EINVAL, "kmpgpu_comm_unique_id: NULL argument");
    static_assert(sizeof(ncclUniqueId) == KMPGPU_COMM_ID_BYTES, "KMPGPU_COMM_ID_BYTES");
    int rc = rccl_load();
    if (rc) return rc;
    ncclUniqueId id;
    { StdoutToStderr guard; RCCL_TRY(g_rccl.GetUniqueId(&id)); }
    memcpy(id_out, &id, sizeof id);
    return KMPGPU_OK;
}

int kmpgpu_comm_init_rank(kmpgpu_comm **out, kmpgpu_ctx *ctx, int n_ranks, int rank, const void *unique_id)
{
    if (!out || !ctx || !unique_id || n_ranks < 1 || rank < 0 || rank >= n_ranks) return fail(KMPGPU_EINVAL, "kmpgpu_comm_init_rank: bad arguments");
    *out = nullptr;
    if (ctx->comm) return fail(KMPGPU_EINVAL, "kmpgpu_comm_init_rank: the context already belongs to a communicator");
    int rc = rccl_load();
    if (rc) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    ncclUniqueId id;
    memcpy(&id, unique_id, sizeof id);
    kmpgpu_comm *k = new (std::nothrow) kmpgpu_comm();
    if (!k) return fail(KMPGPU_ENOMEM, "kmpgpu_comm_init_rank: out of host memory");
    k->ctx.push_back(ctx);
    k->comm.push_back(nullptr);
    k->n_ranks = n_ranks;
    ncclResult_t r;
    { StdoutToStderr guard; r = g_rccl.CommInitRank(&k->comm[0], n_ranks, id, rank); }
    if (r != ncclSuccess) { delete k; return fail(KMPGPU_EHIP, "ncclCommInitRank failed: %s", g_rccl.GetErrorString(r)); }
    k->device.push_back(ctx->device);
    ctx->comm = k;
    *out = k;
    return KMPGPU_OK;
}

int kmpgpu_comm_allreduce_counts(kmpgpu_comm *k)
{
    if (!k) return fail(KMPGPU_EINVAL, "kmpgpu_comm_allreduce_counts: comm is NULL");
    for (kmpgpu_ctx *c : k->ctx)
        if (!c) return fail(KMPGPU_ESTATE, "kmpgpu_comm_allreduce_counts: a context of this communicator has been destroyed");
    const uint32_t n = k->ctx[0]->n_pat;
    for (kmpgpu_ctx *c : k->ctx) {
        if (!c->d_counts) return fail(KMPGPU_ESTATE, "kmpgpu_comm_allreduce_counts: a context has no patterns set");
        if (c->n_pat != n) return fail(KMPGPU_EINVAL, "kmpgpu_comm_allreduce_counts: the contexts hold different numbers of patterns");
    }
    if (n == 0) return KMPGPU_OK;
    RCCL_TRY(g_rccl.GroupStart());
    for (size_t i = 0; i < k->ctx.size(); i++) {
        kmpgpu_ctx *c = k->ctx[i];
        ncclResult_t r = g_rccl.AllReduce(c->d_counts, c->d_counts, n, ncclUint64, ncclSum, k->comm[i], c->stream);
        if (r != ncclSuccess) { (void)g_rccl.GroupEnd(); return fail(KMPGPU_EHIP, "ncclAllReduce failed: %s", g_rccl.GetErrorString(r)); }
    }
    RCCL_TRY(g_rccl.GroupEnd());
    return KMPGPU_OK;
}

void kmpgpu_comm_destroy(kmpgpu_comm *k)
{
    if (!k) return;
    for (size_t i = 0; i < k->comm.size(); i++) {
        if (k->ctx[i]) {                                    /* (a context destroyed earlier has waited for its stream itself) */
            (void)hipSetDevice(k->ctx[i]->device);
            (void)hipStreamSynchronize(k->ctx[i]->stream);
            k->ctx[i]->comm = nullptr;
        }
        if (!k->comm[i]) continue;
        if (i < k->device.size()) (void)hipSetDevice(k->device[i]);
        (void)g_rccl.CommDestroy(k->comm[i]);
    }
    delete k;
}

}  // extern "C"
