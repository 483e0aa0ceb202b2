/*
 * kmp_cli.c -- the reference's command lines on top of the MI355X hot path.
 *
 * Built twice (csrc/Makefile):
 *   bin/serial       ./serial <file.pcap> <string.txt> [udp/tcp]                     serial.c:2-3,33-51
 *   bin/openmp_data  ./openmp_data <file.pcap> <string.txt> thread_number [tcp/udp]  openmp_data.c:1-2,35-54
 * In the second form thread_number is the number of GPU shards: the payloads are split into
 * contiguous ranges the way mpi_dumping.c:149-157 splits them over ranks (N/P each, remainder to
 * shard 0) and the per-shard counts are summed (mpi_dumping.c:202).
 *
 * stdout is byte-compatible with the reference (serial.c:163-169); throughput details go to
 * stderr.  There is no CPU fallback: without a gfx950 device the program fails with exit code 2.
 *
 * KMPGPU_DEVICE_EXTRACT=1: the raw capture is uploaded and the payload extraction
 * (openmp_data.c:128-147, packet_dumping.h:87-188) runs on the GPU (kmpgpu_load_frames).
 *
 * Extension (the reference prints counts only, serial.c:163-166): with the environment variable
 * KMPGPU_OFFSETS_FILE=<path> every match is also written to <path> as "payload,offset,pattern"
 * lines (payload = index among the extracted payloads, pattern = index in the pattern file).
 * KMPGPU_PACKETS_FILE=<path>: which payloads hold which patterns (kmpgpu_scan_alerts over the rows of kmpgpu_scan_packets), one "payload,pattern" line per
 * pair that holds at least one match, sorted by payload, then by pattern (indices as in the offsets file).
 *
 * KMPGPU_RULES_FILE=<rules> with KMPGPU_ALERTS_FILE=<path>: content rules over the patterns (kmpgpu_set_rules, kmpgpu_scan_alerts; the
 * file format is kmp_rules_parse's, kmphost.h: one rule per line, terms are indices into the pattern file, "!" in front of one that
 * must not be in the payload), one "payload,rule" line per payload that a rule matches, sorted by payload, then by rule (rule =
 * index among the rule lines).  One of the two without the other, or a rules file that does not parse: message on stderr, exit 1,
 * before any GPU work.  Both go together with KMPGPU_NOCASE, KMPGPU_WHOLE_PAYLOAD, KMPGPU_DEVICE_EXTRACT and KMPGPU_PACKETS_FILE.
 *
 * KMPGPU_RELATIONS_FILE=<relations>, together with KMPGPU_RULES_FILE and KMPGPU_ALERTS_FILE: distance / within relations between two
 * patterns (kmpgpu_set_relations; the file format is kmp_relations_parse's, kmphost.h: "<a> <b> <dmin> <dmax>" per line, '*' for an
 * unbounded side), set on every shard's context before the rules, whose file may then name relation q as "r<q>" / "!r<q>"
 * (kmp_rules_parse_rel).  A relations file that does not parse, or the variable without the other two: message on stderr, exit 1,
 * before any GPU work.  stdout is what it is without the variable.
 *
 * KMPGPU_CHAINS_FILE=<chains>, together with KMPGPU_RULES_FILE and KMPGPU_ALERTS_FILE, with or without KMPGPU_RELATIONS_FILE: content
 * chains, each content relative to the match before it (kmpgpu_set_chains; the file format is kmp_chains_parse's, kmphost.h:
 * "<p0> <dmin> <dmax> <p1> [<dmin> <dmax> <p2> ...]" per line), set on every shard's context behind the relations and before the rules,
 * whose file may then name chain q as "c<q>" / "!c<q>" (kmp_rules_parse_terms).  A chains file that does not parse, or the variable
 * without the other two: message on stderr, exit 1, before any GPU work.  stdout is what it is without the variable.
 *
 * KMPGPU_WINDOWS_FILE=<windows>: per-pattern offset windows (kmpgpu_set_windows; the file format is kmp_windows_parse's, kmphost.h:
 * "<pattern index> <first> <last>" per line, '*' for no upper bound) on every shard's context.  They take effect on the files written
 * for KMPGPU_OFFSETS_FILE, KMPGPU_PACKETS_FILE and KMPGPU_RULES_FILE + KMPGPU_ALERTS_FILE: only the matches that start inside their
 * pattern's window are listed, mark a payload or feed a rule.  stdout -- the counts -- is what it is without windows.  A windows
 * file that does not parse, or one set without any of those output files (it has no effect): message on stderr, exit 1, before
 * any GPU work.
 *
 * KMPGPU_EXPORT_FILE=<out.pcap>: the payloads that hold at least one pattern (any of kmpgpu_scan_packets) -- with KMPGPU_RULES_FILE set,
 * the payloads that at least one rule matches (any of kmpgpu_scan_rules) -- written as a capture, in payload order over all shards.
 * Per shard the selection is compacted on the device into a second context (kmpgpu_load_selected) and only the selected bytes are
 * downloaded.  The frames are the synthetic Ethernet/IPv4/UDP frames of kmp_write_udp_pcap around the payloads, also in tcp mode: the
 * capture's own headers are not kept.  Windows (KMPGPU_WINDOWS_FILE) decide what a hit is here as in the packets file; with
 * KMPGPU_RULES_FILE, KMPGPU_ALERTS_FILE may be left out when this variable is set.  A path that cannot be written: message on stderr,
 * exit 1, before any GPU work.  stdout is what it is without the variable.
 *
 * KMPGPU_NOCASE=1: every pattern matches case-insensitively (ASCII letters; kmpgpu_set_patterns_flags), in the counts and in
 * the offsets file alike; the report prints every token as written in the pattern file.
 *
 * KMPGPU_WHOLE_PAYLOAD=1: a payload is matched up to its end instead of up to its first 0x00 (KMPGPU_OPT_WHOLE_PAYLOAD; not the
 * reference's behaviour), in the counts, the offsets file and the packets file alike; KMPGPU_STATS=1 prints which rule was used.
 * Unset or 0: the reference's rule, output as ever.
 */
#include <errno.h>
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "kmpgpu.h"
#include "kmphost.h"

#ifndef KMP_CLI_OPENMP_FORM
#define KMP_CLI_OPENMP_FORM 0
#endif

#if KMP_CLI_OPENMP_FORM
#define PROG "./openmp_data"
#define ARGS "<file.pcap> <string.txt> thread_number [tcp/udp]"
#else
#define PROG "./serial"
#define ARGS "<file.pcap> <string.txt> [tcp/udp]"
#endif

static double now_s(void)
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

static int parse_proto(const char *s, int *proto)
{
    if (strcmp(s, "udp") == 0) { *proto = KMP_PROTO_UDP; return 1; }       /* serial.c:38-41 */
    if (strcmp(s, "tcp") == 0) { *proto = KMP_PROTO_TCP; return 1; }
    return 0;
}

static void die_gpu(const char *what)
{
    fprintf(stderr, "%s: %s\n", what, kmpgpu_last_error());
    exit(2);
}

/* One "payload,index" line per record of a context's alert list (kmpgpu_scan_alerts: built and sorted by payload, then index, on the
 * device), the payload counted from the shard's first one.  The records come back in pieces of a fixed size; no bit matrix leaves the
 * device. */
#define ALERT_PIECE 65536u
static void write_alerts(FILE *fp, kmpgpu_ctx *ctx, int family, uint64_t shard_lo)
{
    static kmpgpu_alert piece[ALERT_PIECE];
    uint64_t found = 0;
    if (kmpgpu_scan_alerts(ctx, family, UINT64_MAX, &found, NULL, NULL, NULL, NULL)) die_gpu("kmpgpu_scan_alerts");
    for (uint64_t first = 0; first < found; first += ALERT_PIECE) {
        const uint64_t n = found - first < ALERT_PIECE ? found - first : ALERT_PIECE;
        if (kmpgpu_alerts_read(ctx, piece, first, n)) die_gpu("kmpgpu_alerts_read");
        for (uint64_t i = 0; i < n; i++) fprintf(fp, "%llu,%u\n", (unsigned long long)(shard_lo + piece[i].packet), piece[i].index);
    }
}

/* The HIP runtime takes 0.2-0.3 s to come up.  It does so on a side thread while the main thread maps, indexes
 * and extracts the capture; the two meet before the first context is created. */
static void *warm_gpu(void *arg)
{
    (void)arg;
    if (kmpgpu_device_count() > 0) {
        kmpgpu_ctx *w = NULL;
        if (kmpgpu_init(&w, 0) == 0) kmpgpu_destroy(w);
    }
    return NULL;
}

/* One GPU shard: a contiguous range of the payloads (or, with KMPGPU_DEVICE_EXTRACT=1, of the frames). */
typedef struct shard_job {
    int device, tcp, threaded, rc;
    uint64_t lo, cnt;                       /* first unit and number of units of this shard */
    const kmp_arena *arena;
    const kmp_frames *frames;               /* non-NULL: extraction on the device */
    const uint8_t *const *pp;
    const kmp_patterns *pats;
    kmpgpu_ctx *ctx;
    kmpgpu_timing t;
    uint64_t n_payloads, payload_bytes;
    uint64_t *reb, *own;
    const char *what;
    char err[512];
    pthread_t thread;
} shard_job;

/* KMPGPU_WINDOWS_FILE: the windows every shard's context gets behind its patterns (NULL: none) */
static uint32_t *g_win_first, *g_win_last;
/* KMPGPU_RELATIONS_FILE: the relations every shard's context gets behind its patterns, before any rule is set (n == 0: none) */
static kmp_relations g_relations;
/* KMPGPU_CHAINS_FILE: the chains every shard's context gets behind its relations, before any rule is set (n == 0: none) */
static kmp_chains g_chains;

static int whole_payload_env(void)
{
    const char *e = getenv("KMPGPU_WHOLE_PAYLOAD");
    return e && e[0] == '1' && e[1] == 0;
}

/* KMPGPU_NOCASE=1: every pattern is matched case-insensitively (ASCII letters, KMPGPU_PAT_NOCASE); the report prints the
 * tokens as written. */
static int set_patterns_env(kmpgpu_ctx *c, const uint8_t *const *pp, const uint32_t *len, uint32_t n)
{
    /* KMPGPU_WHOLE_PAYLOAD=1: payloads are matched to their ends, not to their first 0x00 (KMPGPU_OPT_WHOLE_PAYLOAD); every context
     * of the run passes through here */
    if (whole_payload_env() && kmpgpu_set_option(c, KMPGPU_OPT_WHOLE_PAYLOAD, 1)) return KMPGPU_EINVAL;
    const char *e = getenv("KMPGPU_NOCASE");
    if (!(e && e[0] == '1' && e[1] == 0) || n == 0) return kmpgpu_set_patterns(c, pp, len, n);
    uint32_t *fl = (uint32_t *)malloc(n * sizeof *fl);
    if (!fl) return KMPGPU_ENOMEM;
    for (uint32_t i = 0; i < n; i++) fl[i] = KMPGPU_PAT_NOCASE;
    const int rc = kmpgpu_set_patterns_flags(c, pp, len, fl, n);
    free(fl);
    return rc;
}

static void *shard_fail(shard_job *j, const char *what)
{
    j->rc = 1; j->what = what;
    snprintf(j->err, sizeof j->err, "%s", kmpgpu_last_error());            /* the error text is per thread */
    return NULL;
}

static void *shard_load(void *arg)
{
    shard_job *j = (shard_job *)arg;
    if (kmpgpu_init(&j->ctx, j->device)) return shard_fail(j, "kmpgpu_init");
    if (set_patterns_env(j->ctx, j->pp, j->pats->len, j->pats->n)) return shard_fail(j, "kmpgpu_set_patterns");
    if (g_win_first && kmpgpu_set_windows(j->ctx, g_win_first, g_win_last, j->pats->n)) return shard_fail(j, "kmpgpu_set_windows");
    _Static_assert(sizeof(kmp_relation) == sizeof(kmpgpu_relation), "kmp_relation has the layout of kmpgpu_relation");
    if (g_relations.n && kmpgpu_set_relations(j->ctx, (const kmpgpu_relation *)g_relations.rel, g_relations.n)) return shard_fail(j, "kmpgpu_set_relations");
    _Static_assert(sizeof(kmp_chain_link) == sizeof(kmpgpu_chain_link), "kmp_chain_link has the layout of kmpgpu_chain_link");
    if (g_chains.n && kmpgpu_set_chains(j->ctx, g_chains.off, (const kmpgpu_chain_link *)g_chains.links, g_chains.n)) return shard_fail(j, "kmpgpu_set_chains");
    if (j->frames) {
        /* only the bytes this shard's frames span are uploaded (kmpgpu_load_frames) */
        if (kmpgpu_load_frames(j->ctx, j->frames->bytes, j->frames->nbytes, j->frames->off + j->lo, j->frames->caplen + j->lo, j->cnt, j->tcp,
                               &j->n_payloads))
            return shard_fail(j, "kmpgpu_load_frames");
        kmpgpu_arena_info(j->ctx, NULL, &j->payload_bytes);
    } else {
        const kmp_arena *a = j->arena;
        const uint64_t hi = j->lo + j->cnt;
        const uint64_t b0 = a->off[j->lo];
        const uint64_t b1 = (hi < a->n_pkts) ? a->off[hi] : a->nbytes;
        j->reb = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)j->cnt);
        if (!j->reb) { j->rc = 1; j->what = "malloc"; snprintf(j->err, sizeof j->err, "out of memory"); return NULL; }
        for (uint64_t k = 0; k < j->cnt; k++) j->reb[k] = a->off[j->lo + k] - b0;
        /* slots are contiguous and at least 16 bytes each, so [b0, b1) holds the whole shard */
        if (kmpgpu_load_arena(j->ctx, a->bytes + b0, b1 - b0, j->reb, a->len + j->lo, j->cnt)) return shard_fail(j, "kmpgpu_load_arena");
    }
    if (kmpgpu_last_timing(j->ctx, &j->t)) return shard_fail(j, "kmpgpu_last_timing");
    return NULL;
}

int main(int argc, char *argv[])
{
    int proto = KMP_PROTO_UDP;                                              /* serial.c:31 */
    int shards = 1;
#if KMP_CLI_OPENMP_FORM
    if (argc == 4 || argc == 5) {                                           /* openmp_data.c:35 */
        shards = atoi(argv[3]);                                             /* openmp_data.c:38 */
        if (argc == 5 && !parse_proto(argv[4], &proto)) {
            printf("USAGE " PROG " " ARGS "\n");                            /* openmp_data.c:46 */
            exit(1);
        }
    } else {
        printf("USAGE: " PROG " " ARGS "\n");                               /* openmp_data.c:52 */
        exit(1);
    }
    if (shards < 1) shards = 1;
#else
    if (argc == 3 || argc == 4) {                                           /* serial.c:33 */
        if (argc == 4 && !parse_proto(argv[3], &proto)) {
            printf("USAGE " PROG " " ARGS "\n");                            /* serial.c:43 */
            exit(1);
        }
    } else {
        printf("USAGE: " PROG " " ARGS "\n");                               /* serial.c:49 */
        exit(1);
    }
#endif
    const char *pcap_path = argv[1], *strings_path = argv[2];

    kmp_patterns pats;
    int rc = kmp_patterns_load(strings_path, &pats);                        /* serial.c:54-87 */
    if (rc == KMPHOST_EIO) {
        perror("error opening file: ");                                     /* serial.c:61 */
        exit(1);
    }
    if (rc) {
        fprintf(stderr, "error reading pattern file: %s\n", rc == KMPHOST_ETOKEN ? "token longer than 99 bytes" : "out of memory");
        exit(1);
    }

    /* the content rules, read before anything touches the GPU */
    const char *rules_path = getenv("KMPGPU_RULES_FILE"), *alerts_path = getenv("KMPGPU_ALERTS_FILE");
    if (rules_path && !rules_path[0]) rules_path = NULL;
    if (alerts_path && !alerts_path[0]) alerts_path = NULL;
    kmp_rules rules;
    memset(&rules, 0, sizeof rules);
    const char *export_path = getenv("KMPGPU_EXPORT_FILE");
    if (export_path && !export_path[0]) export_path = NULL;
    if ((rules_path != NULL) != (alerts_path != NULL) && !(rules_path && export_path)) {      /* (an export takes the rules' any[] without an alerts file) */
        fprintf(stderr, "KMPGPU_RULES_FILE and KMPGPU_ALERTS_FILE go together: %s is not set\n", rules_path ? "KMPGPU_ALERTS_FILE" : "KMPGPU_RULES_FILE");
        exit(1);
    }
    /* the relations, which the rules may name */
    const char *relations_path = getenv("KMPGPU_RELATIONS_FILE");
    if (relations_path && relations_path[0]) {
        if (!rules_path || !alerts_path) {
            fprintf(stderr, "KMPGPU_RELATIONS_FILE goes together with KMPGPU_RULES_FILE and KMPGPU_ALERTS_FILE: %s is not set\n", rules_path ? "KMPGPU_ALERTS_FILE" : "KMPGPU_RULES_FILE");
            exit(1);
        }
        char relations_err[KMP_RELATIONS_ERRBUF];
        if (kmp_relations_parse(relations_path, pats.n, &g_relations, relations_err)) {
            fprintf(stderr, "error reading relations file %s: %s\n", relations_path, relations_err);
            exit(1);
        }
    }
    /* ... and the chains */
    const char *chains_path = getenv("KMPGPU_CHAINS_FILE");
    if (chains_path && chains_path[0]) {
        if (!rules_path || !alerts_path) {
            fprintf(stderr, "KMPGPU_CHAINS_FILE goes together with KMPGPU_RULES_FILE and KMPGPU_ALERTS_FILE: %s is not set\n", rules_path ? "KMPGPU_ALERTS_FILE" : "KMPGPU_RULES_FILE");
            exit(1);
        }
        char chains_err[KMP_CHAINS_ERRBUF];
        if (kmp_chains_parse(chains_path, pats.n, &g_chains, chains_err)) {
            fprintf(stderr, "error reading chains file %s: %s\n", chains_path, chains_err);
            exit(1);
        }
    }
    if (rules_path) {
        char rules_err[KMP_RULES_ERRBUF];
        if (kmp_rules_parse_terms(rules_path, pats.n, g_relations.n, g_chains.n, &rules, rules_err)) {
            fprintf(stderr, "error reading rules file %s: %s\n", rules_path, rules_err);
            exit(1);
        }
    }

    /* the offset windows likewise */
    const char *windows_path = getenv("KMPGPU_WINDOWS_FILE");
    if (windows_path && windows_path[0]) {
        const char *of = getenv("KMPGPU_OFFSETS_FILE"), *pf = getenv("KMPGPU_PACKETS_FILE");
        if (!(of && of[0]) && !(pf && pf[0]) && !alerts_path && !export_path) {
            fprintf(stderr, "KMPGPU_WINDOWS_FILE has no effect without KMPGPU_OFFSETS_FILE, KMPGPU_PACKETS_FILE, KMPGPU_EXPORT_FILE or KMPGPU_RULES_FILE + KMPGPU_ALERTS_FILE\n");
            exit(1);
        }
        char windows_err[KMP_WINDOWS_ERRBUF];
        g_win_first = (uint32_t *)malloc(sizeof(uint32_t) * (pats.n ? pats.n : 1));
        g_win_last = (uint32_t *)malloc(sizeof(uint32_t) * (pats.n ? pats.n : 1));
        if (!g_win_first || !g_win_last) { fprintf(stderr, "error reading windows file %s: out of memory\n", windows_path); exit(1); }
        if (kmp_windows_parse(windows_path, pats.n, g_win_first, g_win_last, windows_err)) {
            fprintf(stderr, "error reading windows file %s: %s\n", windows_path, windows_err);
            exit(1);
        }
    }

    /* the export starts as a capture without frames: a path that cannot be written ends the run here */
    if (export_path && kmp_write_udp_pcap_part(export_path, 0, NULL, NULL, NULL, 0, 0)) {
        perror("KMPGPU_EXPORT_FILE");
        exit(1);
    }

#if !KMP_CLI_OPENMP_FORM
    const double t_start = now_s();                                         /* serial.c:110-111: before the file read */
#endif
    pthread_t warm;
    const int warming = pthread_create(&warm, NULL, warm_gpu, NULL) == 0;
    const double t_load0 = now_s();
    char errbuf[KMP_PCAP_ERRBUF];
    kmp_arena arena;
    kmp_frames frames;
    memset(&arena, 0, sizeof arena);
    memset(&frames, 0, sizeof frames);
    const char *dx = getenv("KMPGPU_DEVICE_EXTRACT");
    const int device_extract = dx && dx[0] == '1';
    /* One-shot buffers stay in ordinary memory: pinning 1.5 GB costs 0.22 s and unpinning 0.15 s, while the
     * host-to-device copy runs at PCIe speed from pageable memory and even straight from the mapped file on the
     * MI355X hosts (profiles/r01_h2d_probe.txt).  Pinned buffers pay off where they are reused (bin/openmp_task). */
    if (device_extract)
        rc = kmp_frames_from_pcap(pcap_path, NULL, NULL, &frames, errbuf);
    else
        rc = kmp_arena_from_pcap(pcap_path, proto, NULL, NULL, &arena, errbuf);                              /* serial.c:91-141 */
    const double t_loaded = now_s();
    if (warming) pthread_join(warm, NULL);                                  /* the runtime is up (or there is none: reported below) */
    const double t_warm = now_s();
    if (rc == KMPHOST_EIO || rc == KMPHOST_EFORMAT) {
        fprintf(stderr, "error reading pcap file: %s\n", errbuf);           /* serial.c:93 */
        exit(1);
    }
    if (rc) {
        fprintf(stderr, "error building the payload arena: %s\n", errbuf[0] ? errbuf : kmpgpu_last_error());
        exit(2);
    }
#if KMP_CLI_OPENMP_FORM
    const double t_start = now_s();                                         /* openmp_data.c:126: after the pre-load */
#endif

    const int ndev = kmpgpu_device_count();
    if (ndev <= 0) die_gpu("no MI355X device");

    uint64_t *counts = (uint64_t *)calloc(pats.n ? pats.n : 1, sizeof(uint64_t));
    uint64_t *part = (uint64_t *)calloc(pats.n ? pats.n : 1, sizeof(uint64_t));
    const uint8_t **pp = (const uint8_t **)malloc(sizeof(uint8_t *) * (pats.n ? pats.n : 1));
    for (uint32_t i = 0; i < pats.n; i++) pp[i] = pats.blob + pats.off[i];

    double kernel_ms = 0, h2d_ms = 0;
    /* KMPGPU_STATS=1: also report the bytes up to the first NUL of every payload (what strlen bounds, serial.c:191);
     * one extra pass over the arena, so it is opt-in and the "Elapsed time" line of a plain run stays comparable */
    const char *stats_env = getenv("KMPGPU_STATS");
    const int want_stats = stats_env && stats_env[0] && stats_env[0] != '0';
    uint64_t eff_bytes = 0, h2d_bytes = 0;
    int reduce_rccl = 0;
    kmpgpu_comm *td_comm = NULL; kmpgpu_ctx **td_ctxs = NULL; shard_job *td_job = NULL; int td_n = 0;      /* torn down after the report */
    const uint64_t units = device_extract ? frames.n : arena.n_pkts;       /* what is split over the shards */
    if (pats.n && units) {
        /* Shards: contiguous ranges, N/P each, the remainder to shard 0 (mpi_dumping.c:149-157); shard r on device
         * r % ndev.  Every shard is brought up by its own host thread -- context, patterns, upload (and extraction) --
         * so that the uploads of the shards run side by side, one PCIe link each (MPI_Scatterv, mpi_dumping.c:161). */
        if ((uint64_t)shards > units) shards = (int)units;
        shard_job *job = (shard_job *)calloc((size_t)shards, sizeof *job);
        uint64_t lo = 0;
        for (int r = 0; r < shards; r++) {
            const uint64_t cnt = units / (uint64_t)shards + (r == 0 ? units % (uint64_t)shards : 0);
            job[r].device = r % ndev; job[r].lo = lo; job[r].cnt = cnt;
            job[r].arena = &arena; job[r].frames = device_extract ? &frames : NULL; job[r].tcp = proto == KMP_PROTO_TCP;
            job[r].pp = pp; job[r].pats = &pats;
            lo += cnt;
        }
        for (int r = 1; r < shards; r++)
            if (pthread_create(&job[r].thread, NULL, shard_load, &job[r]) != 0) { job[r].threaded = 0; shard_load(&job[r]); } else job[r].threaded = 1;
        shard_load(&job[0]);
        for (int r = 1; r < shards; r++) if (job[r].threaded) pthread_join(job[r].thread, NULL);
        for (int r = 0; r < shards; r++) {
            if (job[r].rc) { fprintf(stderr, "%s: %s\n", job[r].what, job[r].err); exit(2); }
            h2d_ms += job[r].t.h2d_ms; h2d_bytes += job[r].t.h2d_bytes;
            if (device_extract) { arena.n_pkts += job[r].n_payloads; arena.payload_bytes += job[r].payload_bytes; }
        }
        if (device_extract) arena.n_frames = frames.n;

        /* The count reduce (mpi_dumping.c:202).  One shard per device: RCCL all-reduce over xGMI of the shards' device
         * counters (kmpgpu_comm_*), then ONE download.  Shards that share a device (more shards than GPUs): host sum.
         * KMPGPU_RCCL=0 forces the host sum, =1 asks for the communicator even with a single shard. */
        const char *rccl_env = getenv("KMPGPU_RCCL");
        kmpgpu_comm *comm = NULL;
        kmpgpu_ctx **ctxs = (kmpgpu_ctx **)calloc((size_t)shards, sizeof *ctxs);
        for (int r = 0; r < shards; r++) ctxs[r] = job[r].ctx;
        if (shards <= ndev && (shards > 1 || (rccl_env && rccl_env[0] == '1')) && !(rccl_env && rccl_env[0] == '0')) {
            /* no communicator is no reason to stop: the shards' own counters are summed on the host instead (below) */
            if (kmpgpu_comm_init(&comm, ctxs, shards)) {
                fprintf(stderr, "[kmpgpu] kmpgpu_comm_init: %s -- summing the shards' counts on the host\n", kmpgpu_last_error());
                comm = NULL;
            } else reduce_rccl = 1;
        }
        const double t_scan0 = now_s();
        /* every shard's pass is enqueued before any result is read, so the GPUs work side by side
         * (mpi_dumping.c:198-202: all ranks count, then one reduce) */
        for (int r = 0; r < shards; r++)
            if (kmpgpu_scan_enqueue(ctxs[r], NULL)) die_gpu("kmpgpu_scan_enqueue");
        if (comm) {
            /* the shards' own counts are kept before they are summed in place: the offset files need them again below, and
             * they are what the host sums should the all-reduce fail (n_patterns x 8 bytes per shard) */
            for (int r = 0; r < shards; r++) {
                job[r].own = (uint64_t *)malloc(sizeof(uint64_t) * (pats.n ? pats.n : 1));
                if (!job[r].own || kmpgpu_counts_read(ctxs[r], job[r].own)) die_gpu("kmpgpu_counts_read");
            }
            int bad = kmpgpu_comm_allreduce_counts(comm) != 0;
            if (!bad) bad = kmpgpu_counts_read(ctxs[0], counts) != 0;                          /* MPI_Reduce root 0 */
            for (int r = 1; r < shards && !bad; r++) bad = kmpgpu_sync(ctxs[r]) != 0;
            if (bad) {
                fprintf(stderr, "[kmpgpu] RCCL all-reduce of the counts: %s -- summing the shards' counts on the host\n", kmpgpu_last_error());
                reduce_rccl = 0;
                for (uint32_t i = 0; i < pats.n; i++) {
                    counts[i] = 0;
                    for (int r = 0; r < shards; r++) counts[i] += job[r].own[i];            /* mpi_dumping.c:202 MPI_SUM */
                }
            }
        } else {
            for (int r = 0; r < shards; r++) {
                if (kmpgpu_counts_read(ctxs[r], part)) die_gpu("kmpgpu_counts_read");
                for (uint32_t i = 0; i < pats.n; i++) counts[i] += part[i];     /* mpi_dumping.c:202 MPI_SUM */
                if (getenv("KMPGPU_OFFSETS_FILE")) {
                    job[r].own = (uint64_t *)malloc(sizeof(uint64_t) * pats.n);
                    memcpy(job[r].own, part, sizeof(uint64_t) * pats.n);
                }
            }
        }
        kernel_ms = (now_s() - t_scan0) * 1e3;                              /* wall time of the concurrent passes + reduce (mpi_dumping.c:206 MPI_MAX) */

        const char *off_path = getenv("KMPGPU_OFFSETS_FILE");
        if (off_path && off_path[0]) {
            FILE *off_fp = fopen(off_path, "w");
            if (!off_fp) { perror("KMPGPU_OFFSETS_FILE"); exit(1); }
            uint64_t shard_lo = 0;                                          /* payload index of the shard's first payload */
            for (int r = 0; r < shards; r++) {
                uint64_t total = 0, found = 0, np = 0;
                for (uint32_t i = 0; i < pats.n; i++) total += job[r].own[i];
                kmpgpu_match *mm = (kmpgpu_match *)malloc(sizeof *mm * (size_t)(total ? total : 1));
                if (!mm || kmpgpu_scan_offsets(ctxs[r], mm, total, &found, NULL)) die_gpu("kmpgpu_scan_offsets");
                for (uint64_t i = 0; i < found && i < total; i++)
                    fprintf(off_fp, "%llu,%u,%u\n", (unsigned long long)(mm[i].packet + shard_lo), mm[i].offset, mm[i].pattern);
                free(mm);
                kmpgpu_arena_info(ctxs[r], &np, NULL);
                shard_lo += np;
            }
            fclose(off_fp);
        }
        const char *pk_path = getenv("KMPGPU_PACKETS_FILE");
        if (pk_path && pk_path[0]) {
            FILE *pk_fp = fopen(pk_path, "w");
            if (!pk_fp) { perror("KMPGPU_PACKETS_FILE"); exit(1); }
            uint64_t shard_lo = 0;                                          /* payload index of the shard's first payload */
            for (int r = 0; r < shards; r++) {
                uint64_t np = 0;
                kmpgpu_arena_info(ctxs[r], &np, NULL);
                write_alerts(pk_fp, ctxs[r], KMPGPU_ALERT_PATTERNS, shard_lo);
                shard_lo += np;
            }
            fclose(pk_fp);
        }
        if (alerts_path) {
            FILE *al_fp = fopen(alerts_path, "w");
            if (!al_fp) { perror("KMPGPU_ALERTS_FILE"); exit(1); }
            uint64_t shard_lo = 0;                                          /* payload index of the shard's first payload */
            for (int r = 0; r < shards && rules.n; r++) {
                uint64_t np = 0;
                kmpgpu_arena_info(ctxs[r], &np, NULL);
                if (kmpgpu_set_rules(ctxs[r], rules.off, rules.terms, rules.n)) die_gpu("kmpgpu_set_rules");
                write_alerts(al_fp, ctxs[r], KMPGPU_ALERT_RULES, shard_lo);
                shard_lo += np;
            }
            fclose(al_fp);
        }
        if (export_path) {
            uint64_t written = 0;                                           /* frames in the file so far */
            for (int r = 0; r < shards; r++) {
                uint64_t np = 0, nsel = 0, nb = 0;
                kmpgpu_arena_info(ctxs[r], &np, NULL);
                const uint64_t W = (np + 63) / 64;
                uint64_t *any = (uint64_t *)calloc((size_t)(W ? W : 1), sizeof(uint64_t));
                if (!any) die_gpu("KMPGPU_EXPORT_FILE: out of memory");
                if (rules_path) {
                    if (rules.n && kmpgpu_set_rules(ctxs[r], rules.off, rules.terms, rules.n)) die_gpu("kmpgpu_set_rules");
                    if (rules.n && kmpgpu_scan_rules(ctxs[r], NULL, any, NULL, NULL, NULL)) die_gpu("kmpgpu_scan_rules");
                } else if (kmpgpu_scan_packets(ctxs[r], NULL, any, NULL, NULL, NULL)) die_gpu("kmpgpu_scan_packets");
                /* the shard's selection, compacted next to it on its device; only these bytes come back */
                kmpgpu_ctx *ex = NULL;
                if (kmpgpu_init(&ex, job[r].device)) die_gpu("kmpgpu_init");
                if (kmpgpu_load_selected(ex, ctxs[r], any, 0, &nsel)) die_gpu("kmpgpu_load_selected");
                free(any);
                if (nsel) {
                    if (kmpgpu_arena_download(ex, NULL, 0, &nb, NULL, NULL)) die_gpu("kmpgpu_arena_download");
                    uint8_t *bytes = (uint8_t *)malloc((size_t)(nb ? nb : 1));
                    uint64_t *off = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)nsel);
                    uint32_t *len = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)nsel);
                    if (!bytes || !off || !len || kmpgpu_arena_download(ex, bytes, nb, &nb, off, len)) die_gpu("kmpgpu_arena_download");
                    if (kmp_write_udp_pcap_part(export_path, 1, bytes, off, len, nsel, written)) { perror("KMPGPU_EXPORT_FILE"); exit(1); }
                    written += nsel;
                    free(bytes); free(off); free(len);
                }
                kmpgpu_destroy(ex);
            }
        }
        for (int r = 0; r < shards && want_stats; r++) {
            uint64_t e = 0;
            if (kmpgpu_effective_bytes(ctxs[r], &e)) die_gpu("kmpgpu_effective_bytes");
            eff_bytes += e;
        }
        /* (teardown after the report: serial.c:159-160 takes the time before it frees anything, :178-180) */
        td_comm = comm; td_ctxs = ctxs; td_job = job; td_n = shards;
    }
    const double t_finish = now_s();                                        /* serial.c:159-160 */

    kmp_report(stdout, &pats, counts, t_finish - t_start);                  /* serial.c:163-169 */
    if (td_comm) kmpgpu_comm_destroy(td_comm);
    for (int r = 0; r < td_n; r++) { kmpgpu_destroy(td_ctxs[r]); free(td_job[r].own); free(td_job[r].reb); }
    free(td_ctxs); free(td_job);

    if (kernel_ms > 0) {
        uint64_t total = 0;
        for (uint32_t i = 0; i < pats.n; i++) total += counts[i];
        const double bytes = (double)arena.payload_bytes * (double)pats.n;
        fprintf(stderr, "[kmpgpu] %llu frames, %llu payloads, %llu payload bytes, %u patterns, %d shard(s) on %d device(s), count reduce: %s, %llu bytes uploaded\n",
                (unsigned long long)arena.n_frames, (unsigned long long)arena.n_pkts, (unsigned long long)arena.payload_bytes,
                pats.n, shards, ndev, reduce_rccl ? "RCCL all-reduce" : (shards > 1 ? "host sum" : "none"), (unsigned long long)h2d_bytes);
        fprintf(stderr, "[kmpgpu] kernel %.3f ms (%.2f GB/s payload x patterns, %.3g matches/s), h2d %.3f ms\n", kernel_ms,
                bytes / (kernel_ms * 1e6), (double)total / (kernel_ms * 1e-3), h2d_ms);
        if (want_stats) {
            fprintf(stderr, "[kmpgpu] text rule: %s\n", whole_payload_env() ? "whole payloads (KMPGPU_WHOLE_PAYLOAD=1)" : "up to a payload's first NUL (the reference's strlen)");
            fprintf(stderr, "[kmpgpu] %llu of the %llu payload bytes lie at or before the first NUL of their payload\n",
                    (unsigned long long)eff_bytes, (unsigned long long)arena.payload_bytes);
            fprintf(stderr, "[kmpgpu] phases: capture -> host buffers %.3f s, waiting for the HIP runtime %.3f s, contexts + upload + scan %.3f s\n",
                    t_loaded - t_load0, t_warm - t_loaded, t_finish - t_warm);
        }
    }
    free(counts); free(part); free(pp);
    kmp_arena_free(&arena);
    kmp_frames_free(&frames);
    kmp_patterns_free(&pats);
    kmp_rules_free(&rules);
    kmp_relations_free(&g_relations);
    kmp_chains_free(&g_chains);
    free(g_win_first); free(g_win_last);
    return 0;
}
