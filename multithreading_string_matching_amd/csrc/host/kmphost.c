/*
 * kmphost.c -- host side of the matcher (include/kmphost.h): pcap savefile reader, payload
 * extraction, pattern loader, arena builder, report.  Plain C, no GPU dependency.  Citations are
 * relative to the reference repository.
 */
#define _GNU_SOURCE
#include "kmphost.h"

#include <errno.h>
#if defined(__SSE2__)
#include <emmintrin.h>
#endif
#include <fcntl.h>
#include <pthread.h>
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#ifdef _OPENMP
#include <omp.h>
#endif

/* ============================ pcap savefile reader =====================================
 * What the reference obtains from libpcap: pcap_open_offline (serial.c:91), pcap_next_ex
 * (serial.c:115).  Classic pcap: 24-byte global header {magic, ver_major, ver_minor, thiszone,
 * sigfigs, snaplen, linktype}, then records {ts_sec, ts_frac, caplen, len} + caplen bytes.
 *
 * The file is mapped, not read: records are handed out (and copied from, by several threads) in
 * place.  One walker serves the record reader, the arena builder, the frame index of the on-device
 * extraction and the batch producer, so that all of them end at the same record of a damaged file. */
typedef struct kmp_view {
    const uint8_t *base;
    uint64_t       size;
    int            mapped;       /* 1: munmap, 0: free (fallback for what cannot be mapped, e.g. a pipe) */
} kmp_view;

static int host_threads(void);

/* A large mapping is walked record by record right after it is made; taking its ~250 000 page faults per GB on
 * one thread costs more than the walk itself, so several threads touch the pages first. */
static void view_prefault(const kmp_view *v)
{
    if (v->size < (64u << 20)) return;
    const int nt = host_threads();
    (void)nt;
    const int64_t pages = (int64_t)((v->size + 4095u) >> 12);
    uint64_t sink = 0;
#pragma omp parallel for num_threads(nt) schedule(static) reduction(+ : sink)
    for (int64_t p = 0; p < pages; p++) sink += v->base[(uint64_t)p << 12];
    __asm__ volatile("" :: "r"(sink));
}

static int view_open(const char *path, kmp_view *v, char errbuf[KMP_PCAP_ERRBUF])
{
    memset(v, 0, sizeof *v);
    if (errbuf) errbuf[0] = 0;
    const int fd = open(path, O_RDONLY);
    if (fd < 0) {
        if (errbuf) snprintf(errbuf, KMP_PCAP_ERRBUF, "%s: %s", path, strerror(errno));
        return KMPHOST_EIO;
    }
    struct stat st;
    if (fstat(fd, &st) == 0 && S_ISREG(st.st_mode)) {
        v->size = (uint64_t)st.st_size;
        if (v->size) {
            void *m = mmap(NULL, (size_t)v->size, PROT_READ, MAP_PRIVATE, fd, 0);
            if (m != MAP_FAILED) {
                (void)madvise(m, (size_t)v->size, MADV_WILLNEED);
                v->base = (const uint8_t *)m; v->mapped = 1;
                close(fd);
                view_prefault(v);
                return KMPHOST_OK;
            }
        } else { close(fd); return KMPHOST_OK; }
    }
    /* not mappable: read it */
    size_t cap = 1u << 20, n = 0;
    uint8_t *buf = (uint8_t *)malloc(cap);
    for (;;) {
        if (!buf) { close(fd); if (errbuf) snprintf(errbuf, KMP_PCAP_ERRBUF, "out of memory"); return KMPHOST_ENOMEM; }
        const ssize_t got = read(fd, buf + n, cap - n);
        if (got < 0) { if (errno == EINTR) continue; free(buf); close(fd); if (errbuf) snprintf(errbuf, KMP_PCAP_ERRBUF, "%s: %s", path, strerror(errno)); return KMPHOST_EIO; }
        if (got == 0) break;
        n += (size_t)got;
        if (n == cap) { cap *= 2; uint8_t *nb = (uint8_t *)realloc(buf, cap); if (!nb) free(buf); buf = nb; }
    }
    close(fd);
    v->base = buf; v->size = n; v->mapped = 0;
    return KMPHOST_OK;
}

static void view_close(kmp_view *v)
{
    if (v->base) { if (v->mapped) munmap((void *)v->base, (size_t)v->size); else free((void *)v->base); }
    memset(v, 0, sizeof *v);
}

/* Worker threads for the copy loops: the CPUs this process may use (affinity, cgroup quota), at most 16 --
 * a memcpy stream per core saturates the memory system well before that. */
static int host_threads(void)
{
    static int cached = 0;
    if (cached) return cached;
    int n = 1;
#ifdef _OPENMP
    n = omp_get_num_procs();
#endif
    FILE *fp = fopen("/sys/fs/cgroup/cpu.max", "r");
    if (fp) {
        char q[32]; long period = 0;
        if (fscanf(fp, "%31s %ld", q, &period) == 2 && strcmp(q, "max") != 0 && period > 0) {
            const long quota = atol(q);
            if (quota > 0 && (quota + period - 1) / period < n) n = (int)((quota + period - 1) / period);
        }
        fclose(fp);
    } else {
        long quota = -1, period = 0;
        FILE *fq = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r"), *fpd = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r");
        if (fq && fpd && fscanf(fq, "%ld", &quota) == 1 && fscanf(fpd, "%ld", &period) == 1 && quota > 0 && period > 0 &&
            (quota + period - 1) / period < n) n = (int)((quota + period - 1) / period);
        if (fq) fclose(fq);
        if (fpd) fclose(fpd);
    }
    const char *e = getenv("KMPHOST_THREADS");
    if (e && atoi(e) > 0) n = atoi(e);
    if (n > 16 && !(e && atoi(e) > 0)) n = 16;
    if (n < 1) n = 1;
    cached = n;
    return n;
}

/* Fork-join over [0, n) with plain threads that exist for the call only.  The copy loops of a streamed capture run between
 * GPU uploads; an OpenMP team would keep spinning on its cores after every loop (libgomp's wait policy, fixed when the library
 * is loaded), and on a host that grants this process a CPU quota those spinning threads are taken out of the share of the
 * threads that feed the GPU. */
typedef void (*kmp_range_fn)(void *arg, int64_t lo, int64_t hi);
typedef struct kmp_range_job { kmp_range_fn fn; void *arg; int64_t lo, hi; } kmp_range_job;
static void *range_thread(void *p) { kmp_range_job *j = (kmp_range_job *)p; j->fn(j->arg, j->lo, j->hi); return NULL; }
static void run_parallel(int64_t n, int nthreads, kmp_range_fn fn, void *arg)
{
    if (nthreads > 64) nthreads = 64;
    if (nthreads < 1 || n < 2 * nthreads) nthreads = 1;
    kmp_range_job job[64];
    pthread_t th[64];
    int started[64];
    for (int t = 0; t < nthreads; t++) {
        job[t].fn = fn; job[t].arg = arg; job[t].lo = n * t / nthreads; job[t].hi = n * (t + 1) / nthreads;
        started[t] = t > 0 && pthread_create(&th[t], NULL, range_thread, &job[t]) == 0;
    }
    for (int t = 0; t < nthreads; t++) if (!started[t]) fn(arg, job[t].lo, job[t].hi);      /* thread 0, and whatever could not be started */
    for (int t = 1; t < nthreads; t++) if (started[t]) pthread_join(th[t], NULL);
}

#define PCAPNG_SHB 0x0A0D0D0Au
#define PCAPNG_BOM 0x1A2B3C4Du

static uint32_t bswap32(uint32_t v) { return __builtin_bswap32(v); }
static uint32_t rd32(const uint8_t *p) { uint32_t v; memcpy(&v, p, 4); return v; }

typedef struct kmp_walk {
    const uint8_t *b;
    uint64_t sz, pos;
    int      swap;          /* file byte order differs from the host's */
    int      ng;            /* pcapng (libpcap's pcap_open_offline reads both formats) */
    uint32_t linktype, snaplen;
    const uint8_t *blk;     /* pcapng: the block walk_next returned a packet from, its lengths checked (kmp_arena_from_pcap_ts reads its time) */
} kmp_walk;

/* The checks pcap_open_offline makes on the file header (message texts as libpcap words them). */
static int walk_init(kmp_walk *w, const uint8_t *b, uint64_t sz, char errbuf[KMP_PCAP_ERRBUF])
{
    memset(w, 0, sizeof *w);
    w->b = b; w->sz = sz;
    if (sz < 24u) {
        if (errbuf) snprintf(errbuf, KMP_PCAP_ERRBUF, "truncated dump file; tried to read %zu file header bytes", (size_t)24);
        return KMPHOST_EIO;
    }
    const uint32_t magic = rd32(b), bom = rd32(b + 8);
    if (magic == 0xA1B2C3D4u || magic == 0xA1B23C4Du) w->swap = 0;
    else if (bswap32(magic) == 0xA1B2C3D4u || bswap32(magic) == 0xA1B23C4Du) w->swap = 1;
    else if (magic == PCAPNG_SHB && (bom == PCAPNG_BOM || bswap32(bom) == PCAPNG_BOM)) { w->ng = 1; w->swap = (bom != PCAPNG_BOM); }
    else {
        if (errbuf) snprintf(errbuf, KMP_PCAP_ERRBUF, "unknown file format");
        return KMPHOST_EFORMAT;
    }
    if (w->ng) { w->snaplen = 0; w->linktype = 1; w->pos = 0; }      /* the block walker starts at the section header */
    else {
        w->snaplen = w->swap ? bswap32(rd32(b + 16)) : rd32(b + 16);
        w->linktype = w->swap ? bswap32(rd32(b + 20)) : rd32(b + 20);
        w->pos = 24;
    }
    return KMPHOST_OK;
}

/* One pcapng block body -> a packet?  1 and the packet, 0 for other blocks, -1 for a damaged one. */
static int pcapng_packet(kmp_walk *w, uint32_t type, uint32_t body, const uint8_t *b, uint32_t *caplen, uint32_t *len, const uint8_t **data)
{
    if ((type == 6u || type == 2u) && body >= 20u) {   /* Enhanced Packet Block / obsolete Packet Block */
        const uint32_t cl = w->swap ? bswap32(rd32(b + 12)) : rd32(b + 12), ln = w->swap ? bswap32(rd32(b + 16)) : rd32(b + 16);
        if (cl > body - 20u) return -1;
        *caplen = cl; *len = ln; *data = b + 20;
        return 1;
    }
    if (type == 3u && body >= 4u) {                    /* Simple Packet Block */
        const uint32_t ln = w->swap ? bswap32(rd32(b)) : rd32(b);
        uint32_t cl = ln;
        if (w->snaplen && cl > w->snaplen) cl = w->snaplen;
        if (cl > body - 4u) cl = body - 4u;
        *caplen = cl; *len = ln; *data = b + 4;
        return 1;
    }
    if (type == 1u && body >= 8u) {                    /* Interface Description Block: link type + snaplen of interface 0 */
        uint16_t lt;
        memcpy(&lt, b, 2);
        if (w->snaplen == 0) {
            w->linktype = w->swap ? (uint32_t)((lt >> 8) | ((lt & 0xFF) << 8)) : lt;
            w->snaplen = w->swap ? bswap32(rd32(b + 4)) : rd32(b + 4);
        }
    }
    return 0;
}

/* pcap_next_ex: 1 = packet (data points into the file), -2 = end of file, -1 = truncated / damaged record. */
static int walk_next(kmp_walk *w, uint32_t *caplen, uint32_t *len, const uint8_t **data)
{
    if (!w->ng) {
        if (w->pos >= w->sz) return -2;                 /* clean end of file */
        if (w->sz - w->pos < 16u) return -1;            /* truncated record header */
        const uint8_t *r = w->b + w->pos;
        const uint32_t cl = w->swap ? bswap32(rd32(r + 8)) : rd32(r + 8);
        const uint32_t ln = w->swap ? bswap32(rd32(r + 12)) : rd32(r + 12);
        if (cl > (64u << 20)) return -1;                /* corrupt record */
        if (w->sz - w->pos - 16u < cl) return -1;       /* truncated packet */
        *caplen = cl; *len = ln; *data = r + 16;
        w->pos += 16u + (uint64_t)cl;
        /* The walk touches 16 bytes per record, one cache line in a new place every time: it is bound by memory latency unless the
         * next headers are asked for early.  Captures are mostly runs of equal-sized records, so the headers 8 and 16 records ahead
         * are guessed from this record's size (a wrong guess costs a useless prefetch). */
        {
            const uint64_t step = 16u + (uint64_t)cl;
            if (w->pos + 16u * step < w->sz) {
                __builtin_prefetch(w->b + w->pos + 8u * step);
                __builtin_prefetch(w->b + w->pos + 16u * step);
            }
        }
        return 1;
    }
    for (;;) {
        if (w->pos >= w->sz) return -2;
        if (w->sz - w->pos < 8u) return -1;
        const uint8_t *h = w->b + w->pos;
        uint32_t type = rd32(h), total = rd32(h + 4);
        if (type == PCAPNG_SHB) {                       /* a new section may change the byte order */
            if (w->sz - w->pos < 12u) return -1;
            const uint32_t bom = rd32(h + 8);
            if (bom == PCAPNG_BOM) w->swap = 0;
            else if (bswap32(bom) == PCAPNG_BOM) w->swap = 1;
            else return -1;
            total = w->swap ? bswap32(total) : total;
            if (total < 16u || (total & 3u)) return -1;
            w->pos += total;                            /* a section header that runs past the end ends the file cleanly, as a seek does */
            w->snaplen = 0;
            continue;
        }
        if (w->swap) { type = bswap32(type); total = bswap32(total); }
        if (total < 12u || (total & 3u) || total > (64u << 20)) return -1;
        const uint32_t body = total - 12u;
        if (w->sz - w->pos - 8u < (uint64_t)body + 4u) return -1;      /* body + trailing length */
        const int r = pcapng_packet(w, type, body, h + 8, caplen, len, data);
        w->blk = h;
        w->pos += total;
        if (r != 0) return r;
    }
}

struct kmp_pcap {
    kmp_view view;
    kmp_walk walk;
};

kmp_pcap *kmp_pcap_open(const char *path, char errbuf[KMP_PCAP_ERRBUF])
{
    kmp_pcap *p = (kmp_pcap *)calloc(1, sizeof *p);
    if (!p) { if (errbuf) snprintf(errbuf, KMP_PCAP_ERRBUF, "out of memory"); return NULL; }
    if (view_open(path, &p->view, errbuf) || walk_init(&p->walk, p->view.base, p->view.size, errbuf)) {
        view_close(&p->view);
        free(p);
        return NULL;
    }
    return p;
}

int kmp_pcap_next(kmp_pcap *p, uint32_t *caplen, uint32_t *len, const uint8_t **data)
{
    return walk_next(&p->walk, caplen, len, data);
}

uint32_t kmp_pcap_linktype(const kmp_pcap *p) { return p->walk.linktype; }

void kmp_pcap_close(kmp_pcap *p)
{
    if (!p) return;
    view_close(&p->view);
    free(p);
}

/* ============================ payload extraction ======================================== */

/* packet_dumping.h:87-139 */
int kmp_extract_udp(const uint8_t *f, uint32_t cl, uint32_t *poff, uint32_t *plen)
{
    if (cl < 14u) return 0;                              /* :94  Ethernet header            */
    uint32_t rest = cl - 14u;
    if (rest < 20u) return 0;                            /* :102 minimal IP header          */
    const uint32_t ihl = (uint32_t)(f[14] & 0x0Fu) << 2; /* :108 no version / EtherType test */
    if (rest < ihl) return 0;                            /* :110                            */
    if (f[14 + 9] != 17u) return 0;                      /* :116 protocol field             */
    rest -= ihl;
    if (rest < 8u) return 0;                             /* :125 UDP header                 */
    *poff = 14u + ihl + 8u;                              /* :133 (sizeof(pointer) == 8)     */
    *plen = rest - 8u;                                   /* :136 everything that was captured */
    return 1;
}

/* packet_dumping.h:150-188; frames on which the reference's unsigned arithmetic would wrap
 * (headers longer than the captured bytes) are rejected instead of crashing. */
int kmp_extract_tcp(const uint8_t *f, uint32_t cl, uint32_t *poff, uint32_t *plen)
{
    if (cl < 15u) return 0;
    const uint32_t size_ip = (uint32_t)(f[14] & 0x0Fu) << 2;    /* :165 */
    if (size_ip < 20u) return 0;                                 /* :166 */
    const uint32_t tcp_at = 14u + size_ip;
    if (cl < tcp_at + 13u) return 0;
    const uint32_t size_tcp = (uint32_t)(f[tcp_at + 12u] >> 4) << 2;   /* :175 */
    if (size_tcp < 20u) return 0;                                /* :176 */
    const uint32_t start = tcp_at + size_tcp;
    if (cl < start) return 0;
    *poff = start;                                               /* :181 */
    *plen = cl - start;                                          /* :184 */
    return 1;
}

/* The header fields both extractors walk past, for a frame the one of `proto` accepts: every byte read lies inside the captured
 * bytes then (udp: cl >= 34 and cl - 14 - ihl >= 8; tcp: ihl >= 20 and cl >= 14 + ihl + 20). */
int kmp_extract_meta(const uint8_t *f, uint32_t cl, int proto, kmp_pkt_meta *out)
{
    uint32_t o, l;
    if (!((proto == KMP_PROTO_TCP) ? kmp_extract_tcp(f, cl, &o, &l) : kmp_extract_udp(f, cl, &o, &l))) return 0;
    const uint32_t at = 14u + ((uint32_t)(f[14] & 0x0Fu) << 2);
    memset(out, 0, sizeof *out);
    out->src_ip = (uint32_t)f[26] << 24 | (uint32_t)f[27] << 16 | (uint32_t)f[28] << 8 | f[29];
    out->dst_ip = (uint32_t)f[30] << 24 | (uint32_t)f[31] << 16 | (uint32_t)f[32] << 8 | f[33];
    out->src_port = (uint16_t)((uint32_t)f[at] << 8 | f[at + 1u]);
    out->dst_port = (uint16_t)((uint32_t)f[at + 2u] << 8 | f[at + 3u]);
    out->proto = f[23];
    return 1;
}

/* The TCP sequence number's place, for a frame the extractor of `proto` accepts: T + 4 .. T + 7 lie inside the captured bytes then
 * (udp: cl - 14 - ihl >= 8; tcp: cl >= 14 + ihl + 20).  For a UDP frame the bytes there are its length and checksum. */
int kmp_extract_tcp_seq(const uint8_t *f, uint32_t cl, int proto, uint32_t *seq)
{
    uint32_t o, l;
    if (!((proto == KMP_PROTO_TCP) ? kmp_extract_tcp(f, cl, &o, &l) : kmp_extract_udp(f, cl, &o, &l))) return 0;
    const uint32_t at = 14u + ((uint32_t)(f[14] & 0x0Fu) << 2) + 4u;
    *seq = (uint32_t)f[at] << 24 | (uint32_t)f[at + 1u] << 16 | (uint32_t)f[at + 2u] << 8 | f[at + 3u];
    return 1;
}

/* ============================ pattern list ============================================== */

static int is_c_space(uint8_t b) { return b == ' ' || (b >= '\t' && b <= '\r'); }

/* serial.c:66 fscanf(fp, "%s", str): tokens are maximal runs of non-whitespace bytes. */
int kmp_patterns_parse(const uint8_t *text, size_t n, kmp_patterns *out)
{
    memset(out, 0, sizeof *out);
    /* pass 1: count and measure */
    uint32_t cnt = 0;
    size_t bytes = 0, i = 0;
    while (i < n) {
        while (i < n && is_c_space(text[i])) i++;
        size_t s = i;
        while (i < n && !is_c_space(text[i])) i++;
        if (i > s) {
            size_t tl = i - s;
            const uint8_t *z = (const uint8_t *)memchr(text + s, 0, tl);   /* strlen() view, serial.c:69 */
            if (z) tl = (size_t)(z - (text + s));
            if (tl > KMP_MAX_PATTERN_LEN) return KMPHOST_ETOKEN;           /* would overflow char str[100] */
            if (tl == 0) continue;
            cnt++; bytes += tl + 1;
        }
    }
    out->blob = (uint8_t *)malloc(bytes ? bytes : 1);
    out->off = (uint32_t *)malloc(sizeof(uint32_t) * (cnt ? cnt : 1));
    out->len = (uint32_t *)malloc(sizeof(uint32_t) * (cnt ? cnt : 1));
    if (!out->blob || !out->off || !out->len) { kmp_patterns_free(out); return KMPHOST_ENOMEM; }
    /* pass 2: copy */
    uint32_t k = 0;
    size_t w = 0;
    i = 0;
    while (i < n) {
        while (i < n && is_c_space(text[i])) i++;
        size_t s = i;
        while (i < n && !is_c_space(text[i])) i++;
        if (i > s) {
            size_t tl = i - s;
            const uint8_t *z = (const uint8_t *)memchr(text + s, 0, tl);
            if (z) tl = (size_t)(z - (text + s));
            if (tl == 0) continue;
            out->off[k] = (uint32_t)w;
            out->len[k] = (uint32_t)tl;
            memcpy(out->blob + w, text + s, tl);
            out->blob[w + tl] = 0;
            w += tl + 1;
            k++;
        }
    }
    out->n = cnt;
    return KMPHOST_OK;
}

int kmp_patterns_load(const char *path, kmp_patterns *out)
{
    memset(out, 0, sizeof *out);
    FILE *fp = fopen(path, "rb");                       /* serial.c:59 */
    if (!fp) return KMPHOST_EIO;
    size_t cap = 1 << 16, n = 0;
    uint8_t *buf = (uint8_t *)malloc(cap);
    if (!buf) { fclose(fp); return KMPHOST_ENOMEM; }
    for (;;) {
        size_t got = fread(buf + n, 1, cap - n, fp);
        n += got;
        if (got == 0) break;
        if (n == cap) {
            uint8_t *nb = (uint8_t *)realloc(buf, cap * 2);
            if (!nb) { free(buf); fclose(fp); return KMPHOST_ENOMEM; }
            buf = nb; cap *= 2;
        }
    }
    fclose(fp);
    int rc = kmp_patterns_parse(buf, n, out);
    free(buf);
    return rc;
}

void kmp_patterns_free(kmp_patterns *p)
{
    if (!p) return;
    free(p->blob); free(p->off); free(p->len);
    memset(p, 0, sizeof *p);
}

/* ============================ text files, line by line ================================== */

/* What the rules, relations, chains, windows, headers, byte tests and expression files share: one entry per line, blank lines and lines whose first non-blank character
 * is '#' skipped.  text_lines opens path and hands every other line to fn -- p at its first non-blank character, end behind its last
 * one (the newline included), lineno counting every line of the file from 1 -- until fn returns something other than KMPHOST_OK,
 * which text_lines then returns.  The message of a file that cannot be opened (KMPHOST_EIO) and the one that goes with
 * KMPHOST_ENOMEM are written here. */
#define KMP_LINE_ERRBUF 256
_Static_assert(KMP_RULES_ERRBUF == KMP_LINE_ERRBUF && KMP_RELATIONS_ERRBUF == KMP_LINE_ERRBUF && KMP_CHAINS_ERRBUF == KMP_LINE_ERRBUF &&
               KMP_WINDOWS_ERRBUF == KMP_LINE_ERRBUF && KMP_HEADERS_ERRBUF == KMP_LINE_ERRBUF && KMP_BYTETESTS_ERRBUF == KMP_LINE_ERRBUF &&
               KMP_REGEXES_ERRBUF == KMP_LINE_ERRBUF, "the seven formats' error buffers have one size");
typedef int (*line_fn)(void *ctx, const char *p, const char *end, size_t lineno, char *errbuf);

static int out_of_memory(char *errbuf)
{
    if (errbuf) snprintf(errbuf, KMP_LINE_ERRBUF, "out of memory");
    return KMPHOST_ENOMEM;
}

static int text_lines(const char *path, line_fn fn, void *ctx, char *errbuf)
{
    FILE *fp = fopen(path, "rb");
    if (!fp) {
        if (errbuf) snprintf(errbuf, KMP_LINE_ERRBUF, "%s: %s", path, strerror(errno));
        return KMPHOST_EIO;
    }
    char *line = NULL;
    size_t line_cap = 0, lineno = 0;
    ssize_t got;
    int rc = KMPHOST_OK;
    while (!rc && (got = getline(&line, &line_cap, fp)) >= 0) {
        lineno++;
        const char *p = line, *end = line + got;
        while (p < end && is_c_space((uint8_t)*p)) p++;
        if (p == end || *p == '#') continue;                           /* blank line, comment */
        rc = fn(ctx, p, end, lineno, errbuf);
    }
    free(line);
    fclose(fp);
    return rc == KMPHOST_ENOMEM ? out_of_memory(errbuf) : rc;
}

/* "line N: " and the message into errbuf; KMPHOST_EINVAL */
__attribute__((format(printf, 3, 4))) static int line_error(char *errbuf, size_t lineno, const char *fmt, ...)
{
    if (errbuf) {
        const int k = snprintf(errbuf, KMP_LINE_ERRBUF, "line %zu: ", lineno);
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(errbuf + k, (size_t)(KMP_LINE_ERRBUF - k), fmt, ap);
        va_end(ap);
    }
    return KMPHOST_EINVAL;
}

/* One field of a relations, chains or windows line at *pp: a decimal number, with a leading '-' where neg_ok, that fits lo..hi, or
 * (star != 0) a lone '*' = star.  Leaves *pp behind the field and the blanks that follow it; on failure *tok / *tok_len name the field for
 * the message. */
static int number_field(const char **pp, const char *end, int neg_ok, int64_t lo, int64_t hi, int64_t star, int64_t *out, const char **tok, int *tok_len)
{
    const char *p = *pp;
    *tok = p;
    const int neg = neg_ok && p < end && *p == '-';
    if (neg) p++;
    int64_t v = 0;
    const char *digits = p;
    while (p < end && *p >= '0' && *p <= '9') { if (v < ((int64_t)1 << 40)) v = v * 10 + (int64_t)(*p - '0'); p++; }
    const char *stop = p;
    while (stop < end && !is_c_space((uint8_t)*stop)) stop++;           /* the whole token, for the message */
    *tok_len = (int)(stop - *tok > 64 ? 64 : stop - *tok);
    if (neg) v = -v;
    int ok = p > digits && stop == p && v >= lo && v <= hi;
    if (!ok && star && stop == *tok + 1 && **tok == '*') { v = star; ok = 1; }
    while (stop < end && is_c_space((uint8_t)*stop)) stop++;
    *pp = stop;
    *out = v;
    return ok;
}

static int rules_push(uint32_t **v, size_t *n, size_t *cap, uint32_t x)
{
    if (*n == *cap) {
        const size_t nc = *cap ? *cap * 2 : 64;
        uint32_t *nv = (uint32_t *)realloc(*v, nc * sizeof(uint32_t));
        if (!nv) return KMPHOST_ENOMEM;
        *v = nv; *cap = nc;
    }
    (*v)[(*n)++] = x;
    return KMPHOST_OK;
}

/* ============================ content rules ============================================= */

typedef struct rules_ctx {
    uint32_t n_patterns, n_relations, n_chains;
    kmp_rules *out;
    size_t n_off, cap_off, n_terms, cap_terms;
    uint32_t n_headers, n_bytetests, n_regexes, n_links;
} rules_ctx;

static int rules_line(void *ctx, const char *p, const char *end, size_t lineno, char *errbuf)
{
    rules_ctx *c = (rules_ctx *)ctx;
    while (p < end) {
        const char *tok = p;
        uint32_t neg = 0, row;
        uint64_t v = 0;
        if (*p == '!') { neg = KMP_RULE_NOT; p++; }
        /* r<q>: relation q, where the caller has relations (without any the token is no term at all, as it always was) */
        const int is_rel = c->n_relations && p < end && *p == 'r';
        /* c<q>: chain q, in the same way */
        const int is_chain = c->n_chains && p < end && *p == 'c';
        /* h<q>: header predicate q, in the same way */
        const int is_hdr = c->n_headers && p < end && *p == 'h';
        /* b<q>: byte test q, in the same way */
        const int is_bt = c->n_bytetests && p < end && *p == 'b';
        /* x<q>: expression q, in the same way */
        const int is_rx = c->n_regexes && p < end && *p == 'x';
        /* l<q>: link q, in the same way */
        const int is_link = c->n_links && p < end && *p == 'l';
        if (is_rel || is_chain || is_hdr || is_bt || is_rx || is_link) p++;
        const char *digits = p;
        while (p < end && *p >= '0' && *p <= '9') { if (v < (1ull << 40)) v = v * 10 + (uint64_t)(*p - '0'); p++; }
        const char *stop = p;
        while (stop < end && !is_c_space((uint8_t)*stop)) stop++;   /* the whole token, for the message */
        if (p == digits && neg && stop == p && !is_rel && !is_chain && !is_hdr && !is_bt && !is_rx && !is_link) return line_error(errbuf, lineno, "'!' without a pattern index");
        if (p == digits || stop != p)
            return line_error(errbuf, lineno, "'%.*s' is not a pattern index%s%s%s%s%s%s", (int)(stop - tok > 64 ? 64 : stop - tok), tok,
                              c->n_relations ? " or r<relation index>" : "", c->n_chains ? " or c<chain index>" : "",
                              c->n_headers ? " or h<header index>" : "", c->n_bytetests ? " or b<byte test index>" : "",
                              c->n_regexes ? " or x<expression index>" : "", c->n_links ? " or l<link index>" : "");
        if (is_link) {
            if (v >= c->n_links) return line_error(errbuf, lineno, "link index %llu, but there are %u links", (unsigned long long)v, c->n_links);
            row = c->n_patterns + c->n_relations + c->n_chains + c->n_headers + c->n_bytetests + c->n_regexes + (uint32_t)v;
        } else if (is_rx) {
            if (v >= c->n_regexes) return line_error(errbuf, lineno, "expression index %llu, but there are %u expressions", (unsigned long long)v, c->n_regexes);
            row = c->n_patterns + c->n_relations + c->n_chains + c->n_headers + c->n_bytetests + (uint32_t)v;
        } else if (is_bt) {
            if (v >= c->n_bytetests) return line_error(errbuf, lineno, "byte test index %llu, but there are %u byte tests", (unsigned long long)v, c->n_bytetests);
            row = c->n_patterns + c->n_relations + c->n_chains + c->n_headers + (uint32_t)v;
        } else if (is_hdr) {
            if (v >= c->n_headers) return line_error(errbuf, lineno, "header index %llu, but there are %u header predicates", (unsigned long long)v, c->n_headers);
            row = c->n_patterns + c->n_relations + c->n_chains + (uint32_t)v;
        } else if (is_chain) {
            if (v >= c->n_chains) return line_error(errbuf, lineno, "chain index %llu, but there are %u chains", (unsigned long long)v, c->n_chains);
            row = c->n_patterns + c->n_relations + (uint32_t)v;
        } else if (is_rel) {
            if (v >= c->n_relations) return line_error(errbuf, lineno, "relation index %llu, but there are %u relations", (unsigned long long)v, c->n_relations);
            row = c->n_patterns + (uint32_t)v;
        } else {
            if (v >= c->n_patterns) return line_error(errbuf, lineno, "pattern index %llu, but there are %u patterns", (unsigned long long)v, c->n_patterns);
            row = (uint32_t)v;
        }
        if (rules_push(&c->out->terms, &c->n_terms, &c->cap_terms, row | neg)) return KMPHOST_ENOMEM;
        while (p < end && is_c_space((uint8_t)*p)) p++;
    }
    if (c->n_terms > 0xFFFFFFFFull) return KMPHOST_EINVAL;
    return rules_push(&c->out->off, &c->n_off, &c->cap_off, (uint32_t)c->n_terms);
}

int kmp_rules_parse(const char *path, uint32_t n_patterns, kmp_rules *out, char errbuf[KMP_RULES_ERRBUF])
{
    return kmp_rules_parse_rel(path, n_patterns, 0, out, errbuf);
}

int kmp_rules_parse_rel(const char *path, uint32_t n_patterns, uint32_t n_relations, kmp_rules *out, char errbuf[KMP_RULES_ERRBUF])
{
    return kmp_rules_parse_terms(path, n_patterns, n_relations, 0, out, errbuf);
}

int kmp_rules_parse_terms(const char *path, uint32_t n_patterns, uint32_t n_relations, uint32_t n_chains, kmp_rules *out, char errbuf[KMP_RULES_ERRBUF])
{
    return kmp_rules_parse_hdr(path, n_patterns, n_relations, n_chains, 0, out, errbuf);
}

int kmp_rules_parse_hdr(const char *path, uint32_t n_patterns, uint32_t n_relations, uint32_t n_chains, uint32_t n_headers, kmp_rules *out,
                        char errbuf[KMP_RULES_ERRBUF])
{
    return kmp_rules_parse_bt(path, n_patterns, n_relations, n_chains, n_headers, 0, out, errbuf);
}

int kmp_rules_parse_bt(const char *path, uint32_t n_patterns, uint32_t n_relations, uint32_t n_chains, uint32_t n_headers, uint32_t n_bytetests,
                       kmp_rules *out, char errbuf[KMP_RULES_ERRBUF])
{
    return kmp_rules_parse_rx(path, n_patterns, n_relations, n_chains, n_headers, n_bytetests, 0, out, errbuf);
}

int kmp_rules_parse_rx(const char *path, uint32_t n_patterns, uint32_t n_relations, uint32_t n_chains, uint32_t n_headers, uint32_t n_bytetests,
                       uint32_t n_regexes, kmp_rules *out, char errbuf[KMP_RULES_ERRBUF])
{
    return kmp_rules_parse_links(path, n_patterns, n_relations, n_chains, n_headers, n_bytetests, n_regexes, 0, out, errbuf);
}

int kmp_rules_parse_links(const char *path, uint32_t n_patterns, uint32_t n_relations, uint32_t n_chains, uint32_t n_headers, uint32_t n_bytetests,
                          uint32_t n_regexes, uint32_t n_links, kmp_rules *out, char errbuf[KMP_RULES_ERRBUF])
{
    memset(out, 0, sizeof *out);
    if (errbuf) errbuf[0] = 0;
    /* a term is a row below 2^31: bit 31 is KMP_RULE_NOT (kmpgpu_set_relations, _chains, _headers, _bytetests and _regexes refuse such a set too) */
    if ((uint64_t)n_patterns + n_relations + n_chains + n_headers + n_bytetests + n_regexes + n_links >= (1ull << 31)) {
        if (errbuf) {
            if (n_links) snprintf(errbuf, KMP_RULES_ERRBUF, "%u patterns + %u relations + %u chains + %u header predicates + %u byte tests + %u expressions + %u links do not fit the 2^31 rows a term can name", n_patterns, n_relations, n_chains, n_headers, n_bytetests, n_regexes, n_links);
            else if (n_regexes) snprintf(errbuf, KMP_RULES_ERRBUF, "%u patterns + %u relations + %u chains + %u header predicates + %u byte tests + %u expressions do not fit the 2^31 rows a term can name", n_patterns, n_relations, n_chains, n_headers, n_bytetests, n_regexes);
            else if (n_bytetests) snprintf(errbuf, KMP_RULES_ERRBUF, "%u patterns + %u relations + %u chains + %u header predicates + %u byte tests do not fit the 2^31 rows a term can name", n_patterns, n_relations, n_chains, n_headers, n_bytetests);
            else if (n_headers) snprintf(errbuf, KMP_RULES_ERRBUF, "%u patterns + %u relations + %u chains + %u header predicates do not fit the 2^31 rows a term can name", n_patterns, n_relations, n_chains, n_headers);
            else if (n_chains) snprintf(errbuf, KMP_RULES_ERRBUF, "%u patterns + %u relations + %u chains do not fit the 2^31 rows a term can name", n_patterns, n_relations, n_chains);
            else snprintf(errbuf, KMP_RULES_ERRBUF, "%u patterns + %u relations do not fit the 2^31 rows a term can name", n_patterns, n_relations);
        }
        return KMPHOST_EINVAL;
    }
    rules_ctx c = {n_patterns, n_relations, n_chains, out, 0, 0, 0, 0, n_headers, n_bytetests, n_regexes, n_links};
    int rc = rules_push(&out->off, &c.n_off, &c.cap_off, 0) ? out_of_memory(errbuf) : text_lines(path, rules_line, &c, errbuf);
    if (rc) {
        kmp_rules_free(out);
        return rc;
    }
    out->n = (uint32_t)(c.n_off - 1);
    return KMPHOST_OK;
}

void kmp_rules_free(kmp_rules *r)
{
    if (!r) return;
    free(r->off); free(r->terms);
    memset(r, 0, sizeof *r);
}

/* ============================ links ===================================================== */

typedef struct links_ctx {
    rules_ctx terms;                      /* the tables a link's term may name: the rules' syntax without links */
    kmp_links *out;
    size_t cap;
} links_ctx;

static int links_line(void *ctx, const char *p, const char *end, size_t lineno, char *errbuf)
{
    links_ctx *c = (links_ctx *)ctx;
    const char *word = p;
    while (p < end && !is_c_space((uint8_t)*p)) p++;
    const size_t wl = (size_t)(p - word);
    if (wl >= KMP_LINK_BUFFER) return line_error(errbuf, lineno, "a buffer word of %zu characters: at most %d", wl, KMP_LINK_BUFFER - 1);
    while (p < end && is_c_space((uint8_t)*p)) p++;
    if (p == end) return line_error(errbuf, lineno, "'%.*s' without a term: a line is <buffer> <term>", (int)wl, word);
    if (*p == '!') return line_error(errbuf, lineno, "a link's term is not negated: the rule that names the link negates it");
    if (*p == 'l') return line_error(errbuf, lineno, "a link's term names no link");
    /* the term through the rules' own line parser, into a rule of its own */
    kmp_rules one;
    memset(&one, 0, sizeof one);
    rules_ctx t = c->terms;
    t.out = &one;
    const int rc = rules_line(&t, p, end, lineno, errbuf);
    const uint32_t row = rc || t.n_terms == 0 ? 0u : one.terms[0];
    const size_t n_terms = t.n_terms;
    kmp_rules_free(&one);
    if (rc) return rc;
    if (n_terms != 1) return line_error(errbuf, lineno, "%zu terms: a link is one term", n_terms);
    kmp_links *o = c->out;
    if (o->n == c->cap) {
        const size_t nc = c->cap ? c->cap * 2 : 16;
        char (*nb)[KMP_LINK_BUFFER] = (char (*)[KMP_LINK_BUFFER])realloc(o->buffer, nc * sizeof *nb);
        if (!nb) return KMPHOST_ENOMEM;
        o->buffer = nb;
        uint32_t *nt = (uint32_t *)realloc(o->term, nc * sizeof *nt);
        if (!nt) return KMPHOST_ENOMEM;
        o->term = nt;
        c->cap = nc;
    }
    if (o->n == 0x7FFFFFFFu) return line_error(errbuf, lineno, "too many links");
    memcpy(o->buffer[o->n], word, wl);
    o->buffer[o->n][wl] = 0;
    o->term[o->n++] = row;
    return KMPHOST_OK;
}

int kmp_links_parse(const char *path, uint32_t n_patterns, uint32_t n_relations, uint32_t n_chains, uint32_t n_headers, uint32_t n_bytetests,
                    uint32_t n_regexes, kmp_links *out, char errbuf[KMP_LINKS_ERRBUF])
{
    _Static_assert(KMP_LINKS_ERRBUF == KMP_LINE_ERRBUF, "the links file's error buffer has the size of the others");
    memset(out, 0, sizeof *out);
    if (errbuf) errbuf[0] = 0;
    links_ctx c;
    memset(&c, 0, sizeof c);
    c.terms.n_patterns = n_patterns; c.terms.n_relations = n_relations; c.terms.n_chains = n_chains;
    c.terms.n_headers = n_headers; c.terms.n_bytetests = n_bytetests; c.terms.n_regexes = n_regexes;
    c.out = out;
    const int rc = text_lines(path, links_line, &c, errbuf);
    if (rc) kmp_links_free(out);
    return rc;
}

void kmp_links_free(kmp_links *l)
{
    if (!l) return;
    free(l->buffer); free(l->term);
    memset(l, 0, sizeof *l);
}

/* ============================ relations ================================================= */

typedef struct relations_ctx {
    uint32_t n_patterns;
    kmp_relations *out;
    size_t n, cap;
} relations_ctx;

static int relations_line(void *ctx, const char *p, const char *end, size_t lineno, char *errbuf)
{
    relations_ctx *c = (relations_ctx *)ctx;
    static const char *const what[4] = {"a pattern index", "a pattern index", "a lower bound or '*'", "an upper bound or '*'"};
    int64_t f[4] = {0, 0, 0, 0};
    for (int k = 0; k < 4; k++) {
        const char *tok;
        int tl;
        if (p == end) return line_error(errbuf, lineno, "%d of the four fields <a> <b> <dmin> <dmax>", k);
        if (!number_field(&p, end, k >= 2, k >= 2 ? INT32_MIN : 0, k >= 2 ? INT32_MAX : 0xFFFFFFFFll, k == 2 ? INT32_MIN : k == 3 ? INT32_MAX : 0, &f[k], &tok, &tl))
            return line_error(errbuf, lineno, "'%.*s' is not %s", tl, tok, what[k]);
    }
    if (p != end) return line_error(errbuf, lineno, "more than the four fields <a> <b> <dmin> <dmax>");
    if (f[0] >= c->n_patterns || f[1] >= c->n_patterns)
        return line_error(errbuf, lineno, "pattern index %lld, but there are %u patterns", (long long)(f[0] >= c->n_patterns ? f[0] : f[1]), c->n_patterns);
    if (f[2] > f[3]) return line_error(errbuf, lineno, "lower bound %lld lies above upper bound %lld", (long long)f[2], (long long)f[3]);
    if (c->n == c->cap) {
        const size_t nc = c->cap ? c->cap * 2 : 64;
        kmp_relation *nv = (kmp_relation *)realloc(c->out->rel, nc * sizeof *nv);
        if (!nv) return KMPHOST_ENOMEM;
        c->out->rel = nv; c->cap = nc;
    }
    const kmp_relation r = {(uint32_t)f[0], (uint32_t)f[1], (int32_t)f[2], (int32_t)f[3]};
    c->out->rel[c->n++] = r;
    return KMPHOST_OK;
}

int kmp_relations_parse(const char *path, uint32_t n_patterns, kmp_relations *out, char errbuf[KMP_RELATIONS_ERRBUF])
{
    memset(out, 0, sizeof *out);
    if (errbuf) errbuf[0] = 0;
    relations_ctx c = {n_patterns, out, 0, 0};
    int rc = text_lines(path, relations_line, &c, errbuf);
    if (!rc && c.n > 0x7FFFFFFFull) rc = KMPHOST_EINVAL;
    if (rc) {
        kmp_relations_free(out);
        return rc;
    }
    out->n = (uint32_t)c.n;
    return KMPHOST_OK;
}

void kmp_relations_free(kmp_relations *r)
{
    if (!r) return;
    free(r->rel);
    memset(r, 0, sizeof *r);
}

/* ============================ chains ==================================================== */

typedef struct chains_ctx {
    uint32_t n_patterns;
    kmp_chains *out;
    size_t n_off, cap_off, n_links, cap_links;
} chains_ctx;

static int chains_line(void *ctx, const char *p, const char *end, size_t lineno, char *errbuf)
{
    chains_ctx *c = (chains_ctx *)ctx;
    static const char *const what[3] = {"a pattern index", "a lower bound or '*'", "an upper bound or '*'"};
    kmp_chain_link l[KMP_CHAIN_MAX];
    uint32_t n = 0;                                                 /* contents so far */
    int k = 0;                                                      /* the field that comes next: 0 an index, 1 dmin, 2 dmax */
    int64_t lo = INT32_MIN, hi = INT32_MAX;                         /* the bounds in front of the next index (the first has none) */
    while (p < end) {
        const char *tok;
        int tl;
        int64_t v;
        if (k == 0 && n == KMP_CHAIN_MAX) return line_error(errbuf, lineno, "more than %d contents", KMP_CHAIN_MAX);
        if (!number_field(&p, end, k != 0, k ? INT32_MIN : 0, k ? INT32_MAX : 0xFFFFFFFFll, k == 1 ? INT32_MIN : k == 2 ? INT32_MAX : 0, &v, &tok, &tl))
            return line_error(errbuf, lineno, "'%.*s' is not %s", tl, tok, what[k]);
        if (k == 0) {
            if (v >= c->n_patterns) return line_error(errbuf, lineno, "pattern index %lld, but there are %u patterns", (long long)v, c->n_patterns);
            l[n].pattern = (uint32_t)v; l[n].dmin = (int32_t)lo; l[n].dmax = (int32_t)hi;
            n++; k = 1;
        } else if (k == 1) {
            lo = v; k = 2;
        } else {
            hi = v; k = 0;
            if (lo > hi) return line_error(errbuf, lineno, "lower bound %lld lies above upper bound %lld", (long long)lo, (long long)hi);
        }
    }
    if (k != 1)                                                     /* the line has to end behind an index */
        return line_error(errbuf, lineno, "the fields are <p0> <dmin> <dmax> <p1> [<dmin> <dmax> <p2> ...]: bounds without the content behind them");
    if (n < 2) return line_error(errbuf, lineno, "a chain has at least 2 contents: <p0> <dmin> <dmax> <p1> ...");
    if (c->n_links + n > c->cap_links) {
        const size_t nc = c->cap_links ? c->cap_links * 2 : 64;
        kmp_chain_link *nv = (kmp_chain_link *)realloc(c->out->links, nc * sizeof *nv);
        if (!nv) return KMPHOST_ENOMEM;
        c->out->links = nv; c->cap_links = nc;
    }
    memcpy(c->out->links + c->n_links, l, n * sizeof l[0]);
    c->n_links += n;
    if (c->n_links > 0xFFFFFFFFull) return KMPHOST_EINVAL;
    return rules_push(&c->out->off, &c->n_off, &c->cap_off, (uint32_t)c->n_links);
}

int kmp_chains_parse(const char *path, uint32_t n_patterns, kmp_chains *out, char errbuf[KMP_CHAINS_ERRBUF])
{
    memset(out, 0, sizeof *out);
    if (errbuf) errbuf[0] = 0;
    chains_ctx c = {n_patterns, out, 0, 0, 0, 0};
    int rc = rules_push(&out->off, &c.n_off, &c.cap_off, 0) ? out_of_memory(errbuf) : text_lines(path, chains_line, &c, errbuf);
    if (!rc && c.n_off - 1 > 0x7FFFFFFFull) rc = KMPHOST_EINVAL;
    if (rc) {
        kmp_chains_free(out);
        return rc;
    }
    out->n = (uint32_t)(c.n_off - 1);
    return KMPHOST_OK;
}

void kmp_chains_free(kmp_chains *c)
{
    if (!c) return;
    free(c->off); free(c->links);
    memset(c, 0, sizeof *c);
}

/* ============================ offset windows ============================================ */

typedef struct windows_ctx {
    uint32_t n_patterns, *first, *last;
    uint8_t *named;                                                 /* [n_patterns]: the pattern has a line already */
} windows_ctx;

static int windows_line(void *ctx, const char *p, const char *end, size_t lineno, char *errbuf)
{
    windows_ctx *c = (windows_ctx *)ctx;
    static const char *const what[3] = {"a pattern index", "a first offset", "a last offset or '*'"};
    uint32_t f[3] = {0, 0, 0};
    for (int k = 0; k < 3; k++) {
        const char *tok;
        int tl;
        int64_t v = 0;
        if (p == end) return line_error(errbuf, lineno, "%d of the three fields <pattern index> <first> <last>", k);
        if (!number_field(&p, end, 0, 0, 0xFFFFFFFFll, k == 2 ? 0xFFFFFFFFll : 0, &v, &tok, &tl))      /* '*': UINT32_MAX */
            return line_error(errbuf, lineno, "'%.*s' is not %s", tl, tok, what[k]);
        f[k] = (uint32_t)v;
    }
    if (p != end) return line_error(errbuf, lineno, "more than the three fields <pattern index> <first> <last>");
    if (f[0] >= c->n_patterns) return line_error(errbuf, lineno, "pattern index %u, but there are %u patterns", f[0], c->n_patterns);
    if (f[1] > f[2]) return line_error(errbuf, lineno, "first offset %u lies behind last offset %u", f[1], f[2]);
    if (c->named[f[0]]) return line_error(errbuf, lineno, "pattern %u has a window already", f[0]);
    c->named[f[0]] = 1; c->first[f[0]] = f[1]; c->last[f[0]] = f[2];
    return KMPHOST_OK;
}

int kmp_windows_parse(const char *path, uint32_t n_patterns, uint32_t *first_out, uint32_t *last_out, char errbuf[KMP_WINDOWS_ERRBUF])
{
    if (errbuf) errbuf[0] = 0;
    windows_ctx c = {n_patterns, first_out, last_out, (uint8_t *)calloc(n_patterns ? n_patterns : 1, 1)};
    if (!c.named) return out_of_memory(errbuf);
    for (uint32_t i = 0; i < n_patterns; i++) { first_out[i] = 0u; last_out[i] = 0xFFFFFFFFu; }
    const int rc = text_lines(path, windows_line, &c, errbuf);
    free(c.named);
    return rc;
}

/* ============================ header predicates ========================================= */

typedef struct headers_ctx {
    kmp_headers *out;
    size_t n, cap;
} headers_ctx;

/* the next blank-separated field of a line: 0 at its end */
static int next_field(const char **pp, const char *end, const char **tok, int *len)
{
    const char *p = *pp;
    while (p < end && is_c_space((uint8_t)*p)) p++;
    if (p == end) { *pp = p; return 0; }
    *tok = p;
    while (p < end && !is_c_space((uint8_t)*p)) p++;
    *len = (int)(p - *tok);
    *pp = p;
    return 1;
}

static int field_is(const char *tok, int len, const char *word) { return (int)strlen(word) == len && memcmp(tok, word, (size_t)len) == 0; }

/* decimal digits only, at least one, value <= max */
static int plain_number(const char *p, const char *end, uint64_t max, uint64_t *out)
{
    if (p == end) return 0;
    uint64_t v = 0;
    for (; p < end; p++) {
        if (*p < '0' || *p > '9') return 0;
        v = v * 10 + (uint64_t)(*p - '0');
        if (v > max) return 0;
    }
    *out = v;
    return 1;
}

/* any | n | lo:hi | lo: | :hi over 0..max; 1: a range, 0: not one, -1: lo above hi */
static int range_field(const char *tok, int len, uint64_t max, uint64_t *lo, uint64_t *hi)
{
    *lo = 0; *hi = max;
    if (field_is(tok, len, "any")) return 1;
    const char *end = tok + len, *colon = (const char *)memchr(tok, ':', (size_t)len);
    if (!colon) {
        if (!plain_number(tok, end, max, lo)) return 0;
        *hi = *lo;
        return 1;
    }
    if (len == 1) return 0;                                             /* a lone ':' */
    if (colon > tok && !plain_number(tok, colon, max, lo)) return 0;
    if (colon + 1 < end && !plain_number(colon + 1, end, max, hi)) return 0;
    return *lo > *hi ? -1 : 1;
}

/* any | a.b.c.d | a.b.c.d/n */
static int address_field(const char *tok, int len, uint32_t *ip, uint32_t *mask)
{
    *ip = 0; *mask = 0;
    if (field_is(tok, len, "any")) return 1;
    const char *end = tok + len, *slash = (const char *)memchr(tok, '/', (size_t)len), *p = tok;
    const char *addr_end = slash ? slash : end;
    uint32_t a = 0;
    for (int k = 0; k < 4; k++) {
        const char *dot = k < 3 ? (const char *)memchr(p, '.', (size_t)(addr_end - p)) : addr_end;
        uint64_t v;
        if (!dot || !plain_number(p, dot, 255, &v)) return 0;
        a = a << 8 | (uint32_t)v;
        p = dot + 1;
    }
    uint64_t bits = 32;
    if (slash && !plain_number(slash + 1, end, 32, &bits)) return 0;
    *ip = a;
    *mask = bits ? 0xFFFFFFFFu << (32 - bits) : 0u;
    return 1;
}

static int headers_line(void *ctx, const char *p, const char *end, size_t lineno, char *errbuf)
{
    headers_ctx *c = (headers_ctx *)ctx;
    static const char *const form = "<proto> <src> <sport> <dir> <dst> <dport> [<len>]";
    const char *tok[8];
    int len[8], nf = 0;
    while (nf < 8 && next_field(&p, end, &tok[nf], &len[nf])) nf++;
    if (nf < 6) return line_error(errbuf, lineno, "%d of the six or seven fields %s", nf, form);
    if (nf > 7) return line_error(errbuf, lineno, "more than the seven fields %s", form);
#define FIELD(k) (len[k] > 64 ? 64 : len[k]), tok[k]
    kmp_header h;
    memset(&h, 0, sizeof h);
    uint64_t lo, hi;
    if (field_is(tok[0], len[0], "udp")) h.proto = 17;
    else if (field_is(tok[0], len[0], "tcp")) h.proto = 6;
    else if (field_is(tok[0], len[0], "ip") || field_is(tok[0], len[0], "any")) h.flags |= KMP_HDR_ANY_PROTO;
    else if (plain_number(tok[0], tok[0] + len[0], 255, &lo)) h.proto = (uint8_t)lo;
    else return line_error(errbuf, lineno, "'%.*s' is not a protocol (udp, tcp, ip, any or 0..255)", FIELD(0));
    if (!address_field(tok[1], len[1], &h.src_ip, &h.src_mask)) return line_error(errbuf, lineno, "'%.*s' is not an address (any, a.b.c.d or a.b.c.d/0..32)", FIELD(1));
    if (!address_field(tok[4], len[4], &h.dst_ip, &h.dst_mask)) return line_error(errbuf, lineno, "'%.*s' is not an address (any, a.b.c.d or a.b.c.d/0..32)", FIELD(4));
    if (field_is(tok[3], len[3], "<>")) h.flags |= KMP_HDR_BIDIR;
    else if (!field_is(tok[3], len[3], "->")) return line_error(errbuf, lineno, "'%.*s' is not a direction (-> or <>)", FIELD(3));
    for (int k = 2; k <= 5; k += 3) {
        const int r = range_field(tok[k], len[k], 65535, &lo, &hi);
        if (r == 0) return line_error(errbuf, lineno, "'%.*s' is not a port range (any, n, lo:hi, lo: or :hi within 0..65535)", FIELD(k));
        if (r < 0) return line_error(errbuf, lineno, "'%.*s': port %llu lies above %llu", FIELD(k), (unsigned long long)lo, (unsigned long long)hi);
        if (k == 2) { h.sport_lo = (uint16_t)lo; h.sport_hi = (uint16_t)hi; } else { h.dport_lo = (uint16_t)lo; h.dport_hi = (uint16_t)hi; }
    }
    h.len_lo = 0; h.len_hi = UINT32_MAX;
    if (nf == 7) {
        const int r = range_field(tok[6], len[6], UINT32_MAX, &lo, &hi);
        if (r == 0) return line_error(errbuf, lineno, "'%.*s' is not a length range (any, n, lo:hi, lo: or :hi within 0..4294967295)", FIELD(6));
        if (r < 0) return line_error(errbuf, lineno, "'%.*s': length %llu lies above %llu", FIELD(6), (unsigned long long)lo, (unsigned long long)hi);
        h.len_lo = (uint32_t)lo; h.len_hi = (uint32_t)hi;
    }
#undef FIELD
    if (c->n == c->cap) {
        const size_t nc = c->cap ? c->cap * 2 : 64;
        kmp_header *nv = (kmp_header *)realloc(c->out->hdr, nc * sizeof *nv);
        if (!nv) return KMPHOST_ENOMEM;
        c->out->hdr = nv; c->cap = nc;
    }
    c->out->hdr[c->n++] = h;
    return KMPHOST_OK;
}

int kmp_headers_parse(const char *path, kmp_headers *out, char errbuf[KMP_HEADERS_ERRBUF])
{
    memset(out, 0, sizeof *out);
    if (errbuf) errbuf[0] = 0;
    headers_ctx c = {out, 0, 0};
    int rc = text_lines(path, headers_line, &c, errbuf);
    if (!rc && c.n > 0x7FFFFFFFull) rc = KMPHOST_EINVAL;
    if (rc) {
        kmp_headers_free(out);
        return rc;
    }
    out->n = (uint32_t)c.n;
    return KMPHOST_OK;
}

void kmp_headers_free(kmp_headers *h)
{
    if (!h) return;
    free(h->hdr);
    memset(h, 0, sizeof *h);
}

/* ============================ flow bits ================================================= */

_Static_assert(KMP_FLOWBITS_ERRBUF == KMP_LINE_ERRBUF, "the flow bits' error buffer has the size of the others");

typedef struct flowbits_ctx {
    uint32_t n_rules;
    kmp_flowbits *out;
    size_t n, cap;
} flowbits_ctx;

static int flowbit_name_char(char ch)
{
    return (ch >= 'A' && ch <= 'Z') || (ch >= 'a' && ch <= 'z') || (ch >= '0' && ch <= '9') || ch == '_' || ch == '.' || ch == '-';
}

static int flowbits_line(void *ctx, const char *p, const char *end, size_t lineno, char *errbuf)
{
    static const char *const words[] = {"isset", "isnotset", "set", "unset", "toggle"};       /* KMP_FB_ISSET .. KMP_FB_TOGGLE */
    flowbits_ctx *c = (flowbits_ctx *)ctx;
    kmp_flowbits *o = c->out;
    const char *tok;
    int len, n_words = 0;
    uint64_t rule;
#define FIELD (len > 64 ? 64 : len), tok
    next_field(&p, end, &tok, &len);                                    /* (the line is not blank) */
    if (!plain_number(tok, tok + len, 0xFFFFFFFFull, &rule)) return line_error(errbuf, lineno, "'%.*s' is not a rule index", FIELD);
    if (rule >= c->n_rules) return line_error(errbuf, lineno, "rule %llu of %u", (unsigned long long)rule, c->n_rules);
    while (next_field(&p, end, &tok, &len)) {
        n_words++;
        kmp_flowbit_op op = {(uint32_t)rule, 0u, KMP_FB_NOALERT, 0u};
        if (!field_is(tok, len, "noalert")) {
            const char *colon = (const char *)memchr(tok, ':', (size_t)len);
            uint32_t w = 0;
            while (colon && w < 5u && !field_is(tok, (int)(colon - tok), words[w])) w++;
            if (!colon || w == 5u)
                return line_error(errbuf, lineno, "'%.*s' is none of set:<name> unset:<name> toggle:<name> isset:<name> isnotset:<name> noalert", FIELD);
            const char *name = colon + 1;
            const int nl = (int)(tok + len - name);
            int ok = nl >= 1 && nl < KMP_FLOWBIT_NAME;
            for (int i = 0; ok && i < nl; i++) ok = flowbit_name_char(name[i]);
            if (!ok) return line_error(errbuf, lineno, "'%.*s': a name is 1..%d characters of [A-Za-z0-9_.-]", FIELD, KMP_FLOWBIT_NAME - 1);
            uint32_t b = 0;
            while (b < o->n_bits && !field_is(name, nl, o->names[b])) b++;
            if (b == o->n_bits) {
                if (b == KMP_FLOWBITS_MAX) return line_error(errbuf, lineno, "'%.*s' is name %d: at most %d flow bits", FIELD, KMP_FLOWBITS_MAX + 1, KMP_FLOWBITS_MAX);
                memcpy(o->names[b], name, (size_t)nl);
                o->names[b][nl] = 0;
                o->n_bits++;
            }
            op.bit = b; op.op = w;
            for (size_t j = 0; j < c->n && w <= KMP_FB_ISNOTSET; j++)
                if (o->ops[j].rule == op.rule && o->ops[j].bit == b && o->ops[j].op == (w ^ 1u))
                    return line_error(errbuf, lineno, "rule %u tests %s both set and clear", op.rule, o->names[b]);
        }
        if (c->n == c->cap) {
            const size_t nc = c->cap ? c->cap * 2 : 64;
            kmp_flowbit_op *nv = (kmp_flowbit_op *)realloc(o->ops, nc * sizeof *nv);
            if (!nv) return KMPHOST_ENOMEM;
            o->ops = nv; c->cap = nc;
        }
        o->ops[c->n++] = op;
    }
#undef FIELD
    if (!n_words) return line_error(errbuf, lineno, "rule %llu has no word", (unsigned long long)rule);
    return KMPHOST_OK;
}

/* A cycle among the names -- an edge Y -> X where a rule tests Y and acts on X != Y -- into errbuf as "a -> b -> a"; 0 without one.
 * Depth first from every name, the path kept: an edge back into the path closes a cycle. */
static int flowbits_cycle(const kmp_flowbits *f, char *errbuf)
{
    uint32_t succ[KMP_FLOWBITS_MAX] = {0}, done = 0;
    for (uint32_t i = 0; i < f->n; i++)
        for (uint32_t j = 0; j < f->n; j++)
            if (f->ops[i].rule == f->ops[j].rule && f->ops[i].op <= KMP_FB_ISNOTSET && f->ops[j].op >= KMP_FB_SET && f->ops[j].op <= KMP_FB_TOGGLE &&
                f->ops[i].bit != f->ops[j].bit)
                succ[f->ops[i].bit] |= 1u << f->ops[j].bit;
    for (uint32_t s = 0; s < f->n_bits; s++) {
        uint32_t stack[KMP_FLOWBITS_MAX], next[KMP_FLOWBITS_MAX], depth = 1, on = 1u << s;
        if (done >> s & 1u) continue;
        stack[0] = s; next[0] = 0;
        while (depth) {
            const uint32_t v = stack[depth - 1];
            uint32_t x = next[depth - 1];
            while (x < f->n_bits && (!(succ[v] >> x & 1u) || (done >> x & 1u))) x++;
            next[depth - 1] = x + 1u;
            if (x >= f->n_bits) { done |= 1u << v; on &= ~(1u << v); depth--; continue; }
            if (on >> x & 1u) {
                if (errbuf) {
                    uint32_t i = 0;
                    size_t k = (size_t)snprintf(errbuf, KMP_LINE_ERRBUF, "the flow bits ");
                    while (stack[i] != x) i++;
                    for (; i < depth && k < KMP_LINE_ERRBUF; i++) k += (size_t)snprintf(errbuf + k, KMP_LINE_ERRBUF - k, "%s -> ", f->names[stack[i]]);
                    if (k < KMP_LINE_ERRBUF) k += (size_t)snprintf(errbuf + k, KMP_LINE_ERRBUF - k, "%s form a cycle", f->names[x]);
                }
                return 1;
            }
            stack[depth] = x; next[depth] = 0; on |= 1u << x; depth++;
        }
    }
    return 0;
}

int kmp_flowbits_parse(const char *path, uint32_t n_rules, kmp_flowbits *out, char errbuf[KMP_FLOWBITS_ERRBUF])
{
    _Static_assert(sizeof(kmp_flowbit_op) == 16, "kmp_flowbit_op has the layout of kmpgpu_flowbit_op");
    memset(out, 0, sizeof *out);
    if (errbuf) errbuf[0] = 0;
    flowbits_ctx c = {n_rules, out, 0, 0};
    int rc = text_lines(path, flowbits_line, &c, errbuf);
    if (!rc && c.n > 0x7FFFFFFFull) rc = KMPHOST_EINVAL;
    out->n = rc ? 0u : (uint32_t)c.n;
    if (!rc && flowbits_cycle(out, errbuf)) rc = KMPHOST_EINVAL;
    if (rc) {
        kmp_flowbits_free(out);
        return rc;
    }
    if (out->n_bits == 0) out->n_bits = 1;                              /* noalert alone: one bit nobody names */
    return KMPHOST_OK;
}

void kmp_flowbits_free(kmp_flowbits *f)
{
    if (!f) return;
    free(f->ops);
    memset(f, 0, sizeof *f);
}

/* ============================ rate thresholds =========================================== */

_Static_assert(KMP_THRESHOLDS_ERRBUF == KMP_LINE_ERRBUF, "the thresholds' error buffer has the size of the others");

typedef struct thresholds_ctx {
    uint32_t n_rules;
    kmp_thresholds *out;
    size_t n, cap;
} thresholds_ctx;

/* "<digits>[.<1 to 6 digits>]" as microseconds, exactly: 0 for a field that is no such number, 2 for one above max */
static int seconds_to_us(const char *p, const char *end, uint64_t max, uint64_t *out)
{
    const char *dot = (const char *)memchr(p, '.', (size_t)(end - p));
    const char *ie = dot ? dot : end;
    uint64_t whole = 0, frac = 0;
    if (p == ie) return 0;
    for (const char *q = p; q < ie; q++) {
        if (*q < '0' || *q > '9') return 0;
        if (whole > (max - (uint64_t)(*q - '0')) / 10u) return 2;
        whole = whole * 10u + (uint64_t)(*q - '0');
    }
    if (dot) {
        const int nd = (int)(end - dot - 1);
        if (nd < 1 || nd > 6) return 0;
        for (const char *q = dot + 1; q < end; q++) {
            if (*q < '0' || *q > '9') return 0;
            frac = frac * 10u + (uint64_t)(*q - '0');
        }
        for (int i = nd; i < 6; i++) frac *= 10u;
    }
    if (whole > (max - frac) / 1000000u) return 2;
    *out = whole * 1000000u + frac;
    return 1;
}

static int thresholds_line(void *ctx, const char *p, const char *end, size_t lineno, char *errbuf)
{
    static const char *const tracks[] = {"by_rule", "by_src", "by_dst", "by_flow"};          /* KMP_THR_BY_RULE .. KMP_THR_BY_FLOW */
    static const char *const types[] = {"at_least", "at_most", "exactly"};                   /* KMP_THR_AT_LEAST .. KMP_THR_EXACTLY */
    thresholds_ctx *c = (thresholds_ctx *)ctx;
    const char *tok;
    int len;
    uint64_t rule, count, window = KMP_THR_NO_WINDOW;
    uint32_t track = 0, type = 0;
#define FIELD (len > 64 ? 64 : len), tok
    next_field(&p, end, &tok, &len);                                    /* (the line is not blank) */
    if (!plain_number(tok, tok + len, 0xFFFFFFFFull, &rule)) return line_error(errbuf, lineno, "'%.*s' is not a rule index", FIELD);
    if (rule >= c->n_rules) return line_error(errbuf, lineno, "rule %llu of %u", (unsigned long long)rule, c->n_rules);
    if (!next_field(&p, end, &tok, &len)) return line_error(errbuf, lineno, "rule %llu has no track (by_rule, by_src, by_dst, by_flow)", (unsigned long long)rule);
    while (track < 4u && !field_is(tok, len, tracks[track])) track++;
    if (track == 4u) return line_error(errbuf, lineno, "'%.*s' is none of by_rule by_src by_dst by_flow", FIELD);
    if (!next_field(&p, end, &tok, &len)) return line_error(errbuf, lineno, "rule %llu has no type (at_least, at_most, exactly)", (unsigned long long)rule);
    while (type < 3u && !field_is(tok, len, types[type])) type++;
    if (type == 3u) return line_error(errbuf, lineno, "'%.*s' is none of at_least at_most exactly", FIELD);
    if (!next_field(&p, end, &tok, &len)) return line_error(errbuf, lineno, "rule %llu has no count", (unsigned long long)rule);
    if (!plain_number(tok, tok + len, 0xFFFFFFFFull, &count) || count == 0)
        return line_error(errbuf, lineno, "'%.*s' is not a count in 1..4294967295", FIELD);
    if (!next_field(&p, end, &tok, &len)) return line_error(errbuf, lineno, "rule %llu has no window (seconds, or all)", (unsigned long long)rule);
    if (!field_is(tok, len, "all")) {
        const int ok = seconds_to_us(tok, tok + len, KMP_THR_NO_WINDOW - 1u, &window);
        if (ok == 0) return line_error(errbuf, lineno, "'%.*s' is neither all nor seconds with at most 6 fraction digits", FIELD);
        if (ok == 2) return line_error(errbuf, lineno, "'%.*s' seconds are more than 2^64 - 2 microseconds", FIELD);
        if (window == 0) return line_error(errbuf, lineno, "'%.*s': a window of 0 holds no payload", FIELD);
    }
    if (next_field(&p, end, &tok, &len)) return line_error(errbuf, lineno, "'%.*s' follows the window", FIELD);
#undef FIELD
    if (c->n == c->cap) {
        const size_t nc = c->cap ? c->cap * 2 : 64;
        kmp_threshold *nv = (kmp_threshold *)realloc(c->out->thr, nc * sizeof *nv);
        if (!nv) return out_of_memory(errbuf);
        c->out->thr = nv; c->cap = nc;
    }
    const kmp_threshold t = {(uint32_t)rule, track, type, (uint32_t)count, window};
    c->out->thr[c->n++] = t;
    return KMPHOST_OK;
}

int kmp_thresholds_parse(const char *path, uint32_t n_rules, kmp_thresholds *out, char errbuf[KMP_THRESHOLDS_ERRBUF])
{
    _Static_assert(sizeof(kmp_threshold) == 24, "kmp_threshold has the layout of kmpgpu_threshold");
    memset(out, 0, sizeof *out);
    if (errbuf) errbuf[0] = 0;
    thresholds_ctx c = {n_rules, out, 0, 0};
    int rc = text_lines(path, thresholds_line, &c, errbuf);
    if (!rc && c.n > 0x7FFFFFFFull) {
        rc = KMPHOST_EINVAL;
        if (errbuf) snprintf(errbuf, KMP_LINE_ERRBUF, "%zu thresholds are more than 2147483647", c.n);
    }
    if (rc) {
        kmp_thresholds_free(out);
        return rc;
    }
    out->n = (uint32_t)c.n;
    return KMPHOST_OK;
}

void kmp_thresholds_free(kmp_thresholds *t)
{
    if (!t) return;
    free(t->thr);
    memset(t, 0, sizeof *t);
}

/* ============================ byte tests ================================================ */

typedef struct bytetests_ctx {
    uint32_t n_patterns;
    kmp_bytetests *out;
    size_t n, cap;
} bytetests_ctx;

/* a whole field as a number: decimal or 0x hex, with a leading '-' where neg_ok; |value| <= 2^32 - 1 */
static int bt_number(const char *p, const char *end, int neg_ok, int64_t *out)
{
    const int neg = neg_ok && p < end && *p == '-';
    if (neg) p++;
    const int hex = end - p > 2 && p[0] == '0' && (p[1] == 'x' || p[1] == 'X');
    if (hex) p += 2;
    if (p == end) return 0;
    int64_t v = 0;
    for (; p < end; p++) {
        int d;
        if (*p >= '0' && *p <= '9') d = *p - '0';
        else if (hex && *p >= 'a' && *p <= 'f') d = *p - 'a' + 10;
        else if (hex && *p >= 'A' && *p <= 'F') d = *p - 'A' + 10;
        else return 0;
        v = v * (hex ? 16 : 10) + d;
        if (v > 0xFFFFFFFFll) return 0;
    }
    *out = neg ? -v : v;
    return 1;
}

static int bytetests_line(void *ctx, const char *p, const char *end, size_t lineno, char *errbuf)
{
    bytetests_ctx *c = (bytetests_ctx *)ctx;
    static const char *const form = "<nbytes> <op> <value> <offset> [after <pattern index>] [little] [mask <m>]";
    static const char *const ops[7] = {"=", "!=", "<", ">", "<=", ">=", "&"};      /* KMP_BT_EQ .. KMP_BT_GE, then the bit test */
    const char *tok[10];
    int len[10], nf = 0;
    while (nf < 10 && next_field(&p, end, &tok[nf], &len[nf])) nf++;
    if (nf < 4) return line_error(errbuf, lineno, "%d of the four fields that begin %s", nf, form);
    if (nf > 9) return line_error(errbuf, lineno, "more fields than %s has", form);
#define FIELD(k) (len[k] > 64 ? 64 : len[k]), tok[k]
    kmp_bytetest b;
    memset(&b, 0, sizeof b);
    b.mask = 0xFFFFFFFFu;
    int64_t v;
    if (!bt_number(tok[0], tok[0] + len[0], 0, &v) || v < 1 || v > 4) return line_error(errbuf, lineno, "'%.*s' is not a byte count (1..4)", FIELD(0));
    b.nbytes = (uint8_t)v;
    int op = 0;
    while (op < 7 && !field_is(tok[1], len[1], ops[op])) op++;
    if (op == 7) return line_error(errbuf, lineno, "'%.*s' is not an operator (= != < > <= >= &)", FIELD(1));
    if (!bt_number(tok[2], tok[2] + len[2], 0, &v)) return line_error(errbuf, lineno, "'%.*s' is not a value (0..4294967295, decimal or 0x hex)", FIELD(2));
    b.value = (uint32_t)v;
    int64_t offset;
    if (!bt_number(tok[3], tok[3] + len[3], 1, &offset) || offset < INT32_MIN || offset > INT32_MAX)
        return line_error(errbuf, lineno, "'%.*s' is not an offset (-2147483648..2147483647, decimal or 0x hex)", FIELD(3));
    b.offset = (int32_t)offset;
    int has_after = 0, has_little = 0, has_mask = 0;
    for (int k = 4; k < nf; k++) {
        if (field_is(tok[k], len[k], "little")) {
            if (has_little) return line_error(errbuf, lineno, "'little' twice");
            has_little = 1; b.flags |= KMP_BT_LITTLE;
        } else if (field_is(tok[k], len[k], "after")) {
            if (has_after) return line_error(errbuf, lineno, "'after' twice");
            if (++k == nf) return line_error(errbuf, lineno, "'after' without a pattern index");
            if (!bt_number(tok[k], tok[k] + len[k], 0, &v)) return line_error(errbuf, lineno, "'%.*s' is not a pattern index", FIELD(k));
            if (v >= c->n_patterns) return line_error(errbuf, lineno, "pattern index %lld, but there are %u patterns", (long long)v, c->n_patterns);
            has_after = 1; b.flags |= KMP_BT_RELATIVE; b.anchor = (uint32_t)v;
        } else if (field_is(tok[k], len[k], "mask")) {
            if (has_mask) return line_error(errbuf, lineno, "'mask' twice");
            if (op == 6) return line_error(errbuf, lineno, "'&' takes its mask from <value>: it has no mask clause");
            if (++k == nf) return line_error(errbuf, lineno, "'mask' without a mask");
            if (!bt_number(tok[k], tok[k] + len[k], 0, &v)) return line_error(errbuf, lineno, "'%.*s' is not a mask (0..4294967295, decimal or 0x hex)", FIELD(k));
            has_mask = 1; b.mask = (uint32_t)v;
        } else
            return line_error(errbuf, lineno, "'%.*s' is none of after <pattern index>, little, mask <m>", FIELD(k));
    }
#undef FIELD
    if (!has_after && b.offset < 0) return line_error(errbuf, lineno, "offset %d lies in front of the payload: only a test after a pattern reaches back", b.offset);
    if (op == 6) { b.mask = b.value; b.value = 0; b.op = KMP_BT_NE; } else b.op = (uint8_t)op;
    if (c->n == c->cap) {
        const size_t nc = c->cap ? c->cap * 2 : 64;
        kmp_bytetest *nv = (kmp_bytetest *)realloc(c->out->bt, nc * sizeof *nv);
        if (!nv) return KMPHOST_ENOMEM;
        c->out->bt = nv; c->cap = nc;
    }
    c->out->bt[c->n++] = b;
    return KMPHOST_OK;
}

int kmp_bytetests_parse(const char *path, uint32_t n_patterns, kmp_bytetests *out, char errbuf[KMP_BYTETESTS_ERRBUF])
{
    memset(out, 0, sizeof *out);
    if (errbuf) errbuf[0] = 0;
    bytetests_ctx c = {n_patterns, out, 0, 0};
    int rc = text_lines(path, bytetests_line, &c, errbuf);
    if (!rc && c.n > 0x7FFFFFFFull) rc = KMPHOST_EINVAL;
    if (rc) {
        kmp_bytetests_free(out);
        return rc;
    }
    out->n = (uint32_t)c.n;
    return KMPHOST_OK;
}

void kmp_bytetests_free(kmp_bytetests *b)
{
    if (!b) return;
    free(b->bt);
    memset(b, 0, sizeof *b);
}

/* ============================ expressions =============================================== */

typedef struct regexes_ctx {
    uint32_t n_patterns;
    kmp_regexes *out;
    size_t n, cap, bytes, cap_bytes;
} regexes_ctx;

static int regexes_line(void *ctx, const char *p, const char *end, size_t lineno, char *errbuf)
{
    regexes_ctx *c = (regexes_ctx *)ctx;
    static const char *const form = "/EXPR/[i][s] [with <pattern index>]";
    while (end > p && is_c_space((uint8_t)end[-1])) end--;                /* (the newline, and blanks in front of it) */
    if (*p != '/') return line_error(errbuf, lineno, "an expression line is %s: it starts with '/'", form);
    const char *close = end;
    while (close > p + 1 && close[-1] != '/') close--;                    /* EXPR runs to the last '/' of the line */
    if (close == p + 1) return line_error(errbuf, lineno, "no closing '/': an expression line is %s", form);
    const char *expr = p + 1, *expr_end = close - 1;
    if (expr == expr_end) return line_error(errbuf, lineno, "an empty expression");
    uint32_t flags = 0, gate = 0;
    const char *q = close;
    for (; q < end && !is_c_space((uint8_t)*q); q++) {
        const uint32_t f = *q == 'i' ? KMP_RX_NOCASE : *q == 's' ? KMP_RX_DOTALL : *q == 'e' ? KMP_RX_GROUPS : 0u;
        if (!f) return line_error(errbuf, lineno, "'%c' is not a flag (i: nocase, s: dotall)", *q);
        if (flags & f) return line_error(errbuf, lineno, "flag '%c' twice", *q);
        flags |= f;
    }
    const char *tok;
    int len;
    if (next_field(&q, end, &tok, &len)) {
        if (!field_is(tok, len, "with")) return line_error(errbuf, lineno, "'%.*s' is not 'with <pattern index>'", len > 64 ? 64 : len, tok);
        if (!next_field(&q, end, &tok, &len)) return line_error(errbuf, lineno, "'with' without a pattern index");
        uint64_t v = 0;
        int k = 0;
        for (; k < len && tok[k] >= '0' && tok[k] <= '9'; k++) if (v < (1ull << 40)) v = v * 10 + (uint64_t)(tok[k] - '0');
        if (k == 0 || k != len) return line_error(errbuf, lineno, "'%.*s' is not a pattern index", len > 64 ? 64 : len, tok);
        if (v >= c->n_patterns) return line_error(errbuf, lineno, "pattern index %llu, but there are %u patterns", (unsigned long long)v, c->n_patterns);
        flags |= KMP_RX_GATED; gate = (uint32_t)v;
        if (next_field(&q, end, &tok, &len)) return line_error(errbuf, lineno, "'%.*s' behind the pattern index", len > 64 ? 64 : len, tok);
    }
    if (c->n == c->cap) {
        const size_t nc = c->cap ? c->cap * 2 : 64;
        uint32_t *no = (uint32_t *)realloc(c->out->off, (nc + 1) * sizeof *no);
        if (!no) return KMPHOST_ENOMEM;
        c->out->off = no;
        uint32_t *nf = (uint32_t *)realloc(c->out->flags, nc * sizeof *nf);
        if (!nf) return KMPHOST_ENOMEM;
        c->out->flags = nf;
        uint32_t *ng = (uint32_t *)realloc(c->out->gate, nc * sizeof *ng);
        if (!ng) return KMPHOST_ENOMEM;
        c->out->gate = ng;
        c->cap = nc;
    }
    const size_t m = (size_t)(expr_end - expr);
    if (c->bytes + m > 0x7FFFFFFFull) return line_error(errbuf, lineno, "more than 2^31 bytes of expressions");
    if (c->bytes + m > c->cap_bytes) {
        size_t nb = c->cap_bytes ? c->cap_bytes * 2 : 4096;
        while (nb < c->bytes + m) nb *= 2;
        uint8_t *nv = (uint8_t *)realloc(c->out->bytes, nb);
        if (!nv) return KMPHOST_ENOMEM;
        c->out->bytes = nv; c->cap_bytes = nb;
    }
    memcpy(c->out->bytes + c->bytes, expr, m);
    c->out->off[c->n] = (uint32_t)c->bytes;
    c->bytes += m;
    c->out->off[c->n + 1] = (uint32_t)c->bytes;
    c->out->flags[c->n] = flags;
    c->out->gate[c->n] = gate;
    c->n++;
    return KMPHOST_OK;
}

int kmp_regexes_parse(const char *path, uint32_t n_patterns, kmp_regexes *out, char errbuf[KMP_REGEXES_ERRBUF])
{
    memset(out, 0, sizeof *out);
    if (errbuf) errbuf[0] = 0;
    regexes_ctx c = {n_patterns, out, 0, 0, 0, 0};
    int rc = text_lines(path, regexes_line, &c, errbuf);
    if (!rc && c.n > 0x7FFFFFFFull) rc = KMPHOST_EINVAL;
    if (!rc && c.n) {
        /* what kmpgpu_set_regexes takes: a pointer and a length per expression */
        out->expr = (const uint8_t **)malloc(c.n * sizeof *out->expr);
        out->len = (uint32_t *)malloc(c.n * sizeof *out->len);
        if (!out->expr || !out->len) rc = out_of_memory(errbuf);
        else
            for (size_t q = 0; q < c.n; q++) {
                out->expr[q] = out->bytes + out->off[q];
                out->len[q] = out->off[q + 1] - out->off[q];
            }
    }
    if (rc) {
        kmp_regexes_free(out);
        return rc;
    }
    out->n = (uint32_t)c.n;
    return KMPHOST_OK;
}

void kmp_regexes_free(kmp_regexes *r)
{
    if (!r) return;
    free(r->bytes); free(r->off); free(r->expr); free(r->len); free(r->flags); free(r->gate);
    memset(r, 0, sizeof *r);
}

/* serial.c:217-238 */
void kmp_failure_table(const uint8_t *pat, uint32_t m, int32_t *prefix)
{
    if (!m) return;
    prefix[0] = 0;
    uint32_t k = 0;                                    /* length of the current border */
    for (uint32_t q = 1; q < m; q++) {
        while (k > 0 && pat[k] != pat[q]) k = (uint32_t)prefix[k - 1];
        if (pat[k] == pat[q]) k++;
        prefix[q] = (int32_t)k;
    }
}

/* ============================ arena ===================================================== */

static uint64_t round_up(uint64_t v, uint64_t a) { return (v + a - 1) / a * a; }

uint64_t kmp_arena_layout(const uint32_t *lens, uint32_t fixed_len, uint64_t n, uint32_t slot_align,
                          uint64_t *off_out, uint32_t *len_out)
{
    if (slot_align < KMP_SLOT_ALIGN) slot_align = KMP_SLOT_ALIGN;
    uint64_t pos = 0;
    for (uint64_t k = 0; k < n; k++) {
        const uint32_t l = lens ? lens[k] : fixed_len;
        if (off_out) off_out[k] = pos;
        if (len_out) len_out[k] = l;
        pos += round_up(l ? l : 1, slot_align);         /* an empty payload still owns a slot */
    }
    return pos + KMP_ARENA_SLACK;
}

static int arena_alloc(kmp_arena *a, uint64_t nbytes, uint64_t n, kmp_alloc_fn alloc_fn, kmp_free_fn free_fn, int zero)
{
    memset(a, 0, sizeof *a);
    a->free_fn = alloc_fn ? free_fn : free;
    a->bytes = (uint8_t *)(alloc_fn ? alloc_fn((size_t)nbytes) : aligned_alloc(4096, (size_t)round_up(nbytes, 4096)));
    a->off = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)(n ? n : 1));
    a->len = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)(n ? n : 1));
    if (!a->bytes || !a->off || !a->len) { kmp_arena_free(a); return KMPHOST_ENOMEM; }
    if (zero) memset(a->bytes, 0, (size_t)nbytes);
    a->nbytes = nbytes;
    return KMPHOST_OK;
}

void kmp_arena_free(kmp_arena *a)
{
    if (!a) return;
    if (a->bytes && a->free_fn) a->free_fn(a->bytes);
    free(a->off); free(a->len);
    memset(a, 0, sizeof *a);
}

int kmp_arena_from_payloads(const uint8_t *const *payloads, const uint32_t *lens, uint64_t n,
                            kmp_alloc_fn alloc_fn, kmp_free_fn free_fn, kmp_arena *out)
{
    const uint64_t nbytes = kmp_arena_layout(lens, 0, n, KMP_SLOT_ALIGN, NULL, NULL);
    int rc = arena_alloc(out, nbytes, n, alloc_fn, free_fn, 1);
    if (rc) return rc;
    kmp_arena_layout(lens, 0, n, KMP_SLOT_ALIGN, out->off, out->len);
    for (uint64_t k = 0; k < n; k++) {
        if (lens[k]) memcpy(out->bytes + out->off[k], payloads[k], lens[k]);
        out->payload_bytes += lens[k];
    }
    out->n_pkts = n;
    out->n_frames = n;
    return KMPHOST_OK;
}

/* serial.c:115-141.  Two passes over the savefile: size the arena, then fill it, so the arena is
 * one allocation of the final size (it may be pinned memory). */
/* Every record of the mapped file: where its captured bytes lie.  Sequential (a record's position depends on
 * all the records before it), but it touches 16 bytes per record only. */
typedef struct kmp_index { uint64_t *off; uint32_t *caplen; uint64_t n, cap; } kmp_index;

static int index_push(kmp_index *ix, uint64_t off, uint32_t cl)
{
    if (ix->n == ix->cap) {
        const uint64_t nc = ix->cap ? ix->cap * 2 : 1u << 16;
        uint64_t *no = (uint64_t *)realloc(ix->off, sizeof(uint64_t) * (size_t)nc);
        if (no) ix->off = no;
        uint32_t *nl = (uint32_t *)realloc(ix->caplen, sizeof(uint32_t) * (size_t)nc);
        if (nl) ix->caplen = nl;
        if (!no || !nl) return KMPHOST_ENOMEM;
        ix->cap = nc;
    }
    ix->off[ix->n] = off; ix->caplen[ix->n] = cl; ix->n++;
    return KMPHOST_OK;
}

static int index_file(const kmp_view *v, kmp_index *ix, char errbuf[KMP_PCAP_ERRBUF])
{
    memset(ix, 0, sizeof *ix);
    kmp_walk w;
    int rc = walk_init(&w, v->base, v->size, errbuf);
    if (rc) return rc;
    uint32_t cl, ln;
    const uint8_t *data;
    while (walk_next(&w, &cl, &ln, &data) >= 0)                       /* serial.c:115: -1 and -2 both end the loop */
        if ((rc = index_push(ix, (uint64_t)(data - v->base), cl)) != 0) {
            free(ix->off); free(ix->caplen); memset(ix, 0, sizeof *ix);
            if (errbuf) snprintf(errbuf, KMP_PCAP_ERRBUF, "out of memory");
            return rc;
        }
    return KMPHOST_OK;
}

int kmp_arena_from_pcap(const char *path, int proto, kmp_alloc_fn alloc_fn, kmp_free_fn free_fn,
                        kmp_arena *out, char errbuf[KMP_PCAP_ERRBUF])
{
    return kmp_arena_from_pcap_meta(path, proto, alloc_fn, free_fn, out, errbuf, NULL);
}

/* ... and with meta_out the accepted frames' header fields beside the index (kmp_extract_meta), from malloc */
int kmp_arena_from_pcap_meta(const char *path, int proto, kmp_alloc_fn alloc_fn, kmp_free_fn free_fn,
                             kmp_arena *out, char errbuf[KMP_PCAP_ERRBUF], kmp_pkt_meta **meta_out)
{
    return kmp_arena_from_pcap_seq(path, proto, alloc_fn, free_fn, out, errbuf, meta_out, NULL);
}

/* ... and with seq_out their sequence numbers (kmp_extract_tcp_seq), from malloc as well */
int kmp_arena_from_pcap_seq(const char *path, int proto, kmp_alloc_fn alloc_fn, kmp_free_fn free_fn,
                            kmp_arena *out, char errbuf[KMP_PCAP_ERRBUF], kmp_pkt_meta **meta_out, uint32_t **seq_out)
{
    memset(out, 0, sizeof *out);
    if (meta_out) *meta_out = NULL;
    if (seq_out) *seq_out = NULL;
    kmp_view v;
    kmp_index ix;
    int rc = view_open(path, &v, errbuf);
    if (rc) return rc;
    if ((rc = index_file(&v, &ix, errbuf)) != 0) { view_close(&v); return rc; }
    const int64_t nf = (int64_t)ix.n;
    const int nt = host_threads();
    (void)nt;
    /* the extraction rule for every frame (serial.c:119-122 / openmp_data.c:128-147 do this per packet too) */
    uint32_t *po = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)(nf ? nf : 1));
    uint32_t *pl = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)(nf ? nf : 1));
    uint64_t *dst = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)(nf ? nf : 1));
    if (!po || !pl || !dst) rc = KMPHOST_ENOMEM;
    if (!rc) {
#pragma omp parallel for num_threads(nt) schedule(static)
        for (int64_t f = 0; f < nf; f++) {
            uint32_t o = 0, l = 0;
            const int ok = (proto == KMP_PROTO_TCP) ? kmp_extract_tcp(v.base + ix.off[f], ix.caplen[f], &o, &l)
                                                    : kmp_extract_udp(v.base + ix.off[f], ix.caplen[f], &o, &l);
            po[f] = o; pl[f] = ok ? l : UINT32_MAX;                 /* UINT32_MAX: skipped (serial.c:138-140) */
        }
        uint64_t n = 0, pos = 0, payload = 0;
        for (int64_t f = 0; f < nf; f++) {
            if (pl[f] == UINT32_MAX) continue;
            dst[f] = pos;
            pos += round_up(pl[f] ? pl[f] : 1, KMP_SLOT_ALIGN);
            payload += pl[f];
            n++;
        }
        rc = arena_alloc(out, pos + KMP_ARENA_SLACK, n, alloc_fn, free_fn, 0);
        if (!rc && meta_out) {
            *meta_out = (kmp_pkt_meta *)malloc(sizeof(kmp_pkt_meta) * (size_t)(n ? n : 1));
            if (!*meta_out) { kmp_arena_free(out); rc = KMPHOST_ENOMEM; }
        }
        if (!rc && seq_out) {
            *seq_out = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)(n ? n : 1));
            if (!*seq_out) {
                kmp_arena_free(out); rc = KMPHOST_ENOMEM;
                if (meta_out) { free(*meta_out); *meta_out = NULL; }
            }
        }
        if (!rc) {
            uint64_t k = 0;
            for (int64_t f = 0; f < nf; f++) {
                if (pl[f] == UINT32_MAX) continue;
                out->off[k] = dst[f]; out->len[k] = pl[f];
                if (meta_out) (void)kmp_extract_meta(v.base + ix.off[f], ix.caplen[f], proto, *meta_out + k);
                if (seq_out) (void)kmp_extract_tcp_seq(v.base + ix.off[f], ix.caplen[f], proto, *seq_out + k);
                k++;
            }
            /* payload copies (serial.c:125-127) + zeroed slot padding, one stream per thread */
#pragma omp parallel for num_threads(nt) schedule(static)
            for (int64_t f = 0; f < nf; f++) {
                if (pl[f] == UINT32_MAX) continue;
                const uint64_t slot = round_up(pl[f] ? pl[f] : 1, KMP_SLOT_ALIGN);
                uint8_t *d = out->bytes + dst[f];
                if (pl[f]) memcpy(d, v.base + ix.off[f] + po[f], pl[f]);
                if (slot > pl[f]) memset(d + pl[f], 0, (size_t)(slot - pl[f]));
            }
            memset(out->bytes + pos, 0, KMP_ARENA_SLACK);
            out->n_pkts = n;
            out->n_frames = (uint64_t)nf;
            out->payload_bytes = payload;
        }
    }
    if (rc == KMPHOST_ENOMEM && errbuf) snprintf(errbuf, KMP_PCAP_ERRBUF, "out of memory");
    free(po); free(pl); free(dst);
    free(ix.off); free(ix.caplen);
    view_close(&v);
    return rc;
}

/* The timestamp of the packet walk_next has just returned, in microseconds: a classic record's ts_sec and ts_frac lie in the 16 bytes in
 * front of its data, which walk_next has found inside the file; a pcapng packet comes from the block w->blk, whose leading length
 * walk_next has checked against the file and whose body pcapng_packet has found to hold the 20 bytes in front of the data -- the trailing
 * length word is file data nobody has checked and is not looked at.  An (Enhanced) Packet Block holds the two halves of its 64-bit
 * timestamp behind the interface id -- taken as microseconds, if_tsresol is not parsed.  A Simple Packet Block has no time: 0. */
static uint64_t walk_ts_us(const kmp_walk *w, const uint8_t *data, int nano)
{
    if (!w->ng) {
        const uint32_t sec = w->swap ? bswap32(rd32(data - 16)) : rd32(data - 16), frac = w->swap ? bswap32(rd32(data - 12)) : rd32(data - 12);
        return (uint64_t)sec * 1000000u + (nano ? frac / 1000u : frac);
    }
    const uint8_t *h = w->blk;
    const uint32_t type = w->swap ? bswap32(rd32(h)) : rd32(h);
    if (type != 6u && type != 2u) return 0;
    const uint32_t hi = w->swap ? bswap32(rd32(h + 12)) : rd32(h + 12), lo = w->swap ? bswap32(rd32(h + 16)) : rd32(h + 16);
    return (uint64_t)hi << 32 | lo;
}

/* ... and with ts_out the accepted frames' capture times in microseconds, from malloc: the arena first, then one more walk over the records */
int kmp_arena_from_pcap_ts(const char *path, int proto, kmp_alloc_fn alloc_fn, kmp_free_fn free_fn,
                           kmp_arena *out, char errbuf[KMP_PCAP_ERRBUF], kmp_pkt_meta **meta_out, uint64_t **ts_out)
{
    return kmp_arena_from_pcap_seq_ts(path, proto, alloc_fn, free_fn, out, errbuf, meta_out, NULL, ts_out);
}

int kmp_arena_from_pcap_seq_ts(const char *path, int proto, kmp_alloc_fn alloc_fn, kmp_free_fn free_fn,
                               kmp_arena *out, char errbuf[KMP_PCAP_ERRBUF], kmp_pkt_meta **meta_out, uint32_t **seq_out, uint64_t **ts_out)
{
    if (ts_out) *ts_out = NULL;
    int rc = kmp_arena_from_pcap_seq(path, proto, alloc_fn, free_fn, out, errbuf, meta_out, seq_out);
    if (rc || !ts_out) return rc;
    uint64_t *ts = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)(out->n_pkts ? out->n_pkts : 1));
    kmp_view v;
    if (ts) rc = view_open(path, &v, errbuf);
    else { rc = KMPHOST_ENOMEM; if (errbuf) snprintf(errbuf, KMP_PCAP_ERRBUF, "out of memory"); }
    if (!rc) {
        kmp_walk w;
        rc = walk_init(&w, v.base, v.size, errbuf);
        if (!rc) {
            const uint32_t magic = rd32(v.base);
            const int nano = !w.ng && (magic == 0xA1B23C4Du || bswap32(magic) == 0xA1B23C4Du);
            uint32_t cl, ln, o, l;
            const uint8_t *data;
            uint64_t k = 0;
            while (walk_next(&w, &cl, &ln, &data) >= 0) {
                if (!((proto == KMP_PROTO_TCP) ? kmp_extract_tcp(data, cl, &o, &l) : kmp_extract_udp(data, cl, &o, &l))) continue;
                if (k < out->n_pkts) ts[k] = walk_ts_us(&w, data, nano);
                k++;
            }
            if (k != out->n_pkts) {                     /* (the file changed between the two walks) */
                rc = KMPHOST_EIO;
                if (errbuf) snprintf(errbuf, KMP_PCAP_ERRBUF, "%s changed while it was read", path);
            }
        }
        view_close(&v);
    }
    if (rc) {
        free(ts);
        kmp_arena_free(out);
        if (meta_out) { free(*meta_out); *meta_out = NULL; }
        if (seq_out) { free(*seq_out); *seq_out = NULL; }
        return rc;
    }
    *ts_out = ts;
    return KMPHOST_OK;
}

/* ============================ raw frames (on-device extraction) ========================= */

int kmp_frames_from_pcap(const char *path, kmp_alloc_fn alloc_fn, kmp_free_fn free_fn, kmp_frames *out,
                         char errbuf[KMP_PCAP_ERRBUF])
{
    memset(out, 0, sizeof *out);
    kmp_view v;
    kmp_index ix;
    int rc = view_open(path, &v, errbuf);
    if (rc) return rc;
    if ((rc = index_file(&v, &ix, errbuf)) != 0) { view_close(&v); return rc; }
    if (!alloc_fn && v.mapped) {                        /* hand the mapping itself out */
        out->bytes = (uint8_t *)v.base; out->nbytes = v.size; out->map_len = v.size; out->free_fn = NULL;
        out->off = ix.off; out->caplen = ix.caplen; out->n = ix.n;
        if (!out->off) {
            out->off = (uint64_t *)malloc(sizeof(uint64_t)); out->caplen = (uint32_t *)malloc(sizeof(uint32_t));
            if (!out->off || !out->caplen) { kmp_frames_free(out); return KMPHOST_ENOMEM; }
        }
        return KMPHOST_OK;
    }
    out->free_fn = alloc_fn ? free_fn : free;
    out->nbytes = v.size;
    out->bytes = (uint8_t *)(alloc_fn ? alloc_fn((size_t)v.size + 64) : malloc((size_t)v.size + 64));
    if (!out->bytes) {
        free(ix.off); free(ix.caplen); view_close(&v);
        if (errbuf) snprintf(errbuf, KMP_PCAP_ERRBUF, "out of memory");
        return KMPHOST_ENOMEM;
    }
    /* the file as it is, copied by several threads (the destination is usually pinned memory) */
    const int nt = host_threads();
    (void)nt;
    const uint64_t piece = 4u << 20;
    const int64_t pieces = (int64_t)((v.size + piece - 1) / piece);
#pragma omp parallel for num_threads(nt) schedule(static)
    for (int64_t i = 0; i < pieces; i++) {
        const uint64_t o = (uint64_t)i * piece, l = (v.size - o < piece) ? v.size - o : piece;
        memcpy(out->bytes + o, v.base + o, (size_t)l);
    }
    memset(out->bytes + v.size, 0, 64);
    out->off = ix.off; out->caplen = ix.caplen; out->n = ix.n;
    if (!out->off) {                                     /* no record: keep the arrays non-NULL */
        out->off = (uint64_t *)malloc(sizeof(uint64_t)); out->caplen = (uint32_t *)malloc(sizeof(uint32_t));
        if (!out->off || !out->caplen) { kmp_frames_free(out); view_close(&v); return KMPHOST_ENOMEM; }
    }
    view_close(&v);
    return KMPHOST_OK;
}

void kmp_frames_free(kmp_frames *f)
{
    if (!f) return;
    if (f->bytes && f->map_len) munmap(f->bytes, (size_t)f->map_len);
    else if (f->bytes && f->free_fn) f->free_fn(f->bytes);
    free(f->off); free(f->caplen);
    memset(f, 0, sizeof *f);
}

/* ============================ streamed capture: batches =================================
 * The producer half of openmp_task.c:126-155. */
struct kmp_batch_reader {
    kmp_view  view;
    kmp_walk  walk;
    int       proto;
    int       pending;          /* a payload has been found but did not fit into the previous batch */
    uint64_t  p_src;            /* its bytes in the file, its length */
    uint32_t  p_len;
    int       eof;
    uint64_t *src;              /* scratch: source offset of every payload of the batch being built */
    uint64_t  src_cap;
};

kmp_batch_reader *kmp_batch_open(const char *path, int proto, char errbuf[KMP_PCAP_ERRBUF])
{
    kmp_batch_reader *r = (kmp_batch_reader *)calloc(1, sizeof *r);
    if (!r) { if (errbuf) snprintf(errbuf, KMP_PCAP_ERRBUF, "out of memory"); return NULL; }
    if (view_open(path, &r->view, errbuf) || walk_init(&r->walk, r->view.base, r->view.size, errbuf)) {
        view_close(&r->view);
        free(r);
        return NULL;
    }
    r->proto = proto;
    return r;
}

typedef struct batch_copy_job { uint8_t *arena; const uint8_t *file; const uint64_t *src, *off; const uint32_t *len; } batch_copy_job;
static void batch_copy_range(void *arg, int64_t lo, int64_t hi)
{
    const batch_copy_job *j = (const batch_copy_job *)arg;
    for (int64_t k = lo; k < hi; k++) {
        const uint64_t slot = round_up(j->len[k] ? j->len[k] : 1, KMP_SLOT_ALIGN);
        uint8_t *d = j->arena + j->off[k];
        if (j->len[k]) memcpy(d, j->file + j->src[k], j->len[k]);
        if (slot > j->len[k]) memset(d + j->len[k], 0, (size_t)(slot - j->len[k]));
    }
}

int64_t kmp_batch_next(kmp_batch_reader *r, uint8_t *arena, uint64_t cap_bytes, uint64_t *off, uint32_t *len,
                       uint64_t cap_pkts, uint64_t *used_bytes, uint64_t *frames)
{
    uint64_t n = 0, pos = 0;
    if (cap_bytes < KMP_ARENA_SLACK + KMP_SLOT_ALIGN) return KMPHOST_EINVAL;
    const uint64_t room = cap_bytes - KMP_ARENA_SLACK;
    /* 1: walk the records and lay the batch out (sequential: headers only) */
    while (!r->eof) {
        if (!r->pending) {
            uint32_t cl, ln, po, pl;
            const uint8_t *data;
            if (walk_next(&r->walk, &cl, &ln, &data) < 0) { r->eof = 1; break; }          /* openmp_task.c:135 */
            if (frames) (*frames)++;
            const int ok = (r->proto == KMP_PROTO_TCP) ? kmp_extract_tcp(data, cl, &po, &pl)
                                                       : kmp_extract_udp(data, cl, &po, &pl);   /* openmp_task.c:139-142 */
            if (!ok) continue;                          /* invalid frames cannot match anything (openmp_task.c:150-153 stores " ") */
            r->p_src = (uint64_t)(data - r->view.base) + po; r->p_len = pl; r->pending = 1;
        }
        const uint64_t slot = round_up(r->p_len ? r->p_len : 1, KMP_SLOT_ALIGN);
        if (slot > room) return KMPHOST_EINVAL;
        if (pos + slot > room || n == cap_pkts) break;                /* keep the payload for the next batch */
        if (n == r->src_cap) {
            const uint64_t nc = r->src_cap ? r->src_cap * 2 : 1u << 16;
            uint64_t *ns = (uint64_t *)realloc(r->src, sizeof(uint64_t) * (size_t)nc);
            if (!ns) return KMPHOST_ENOMEM;
            r->src = ns; r->src_cap = nc;
        }
        r->src[n] = r->p_src;
        off[n] = pos; len[n] = r->p_len;
        pos += slot; n++;
        r->pending = 0;
    }
    /* 2: copy the payloads, several threads (the arena is usually pinned memory) */
    batch_copy_job bj = {arena, r->view.base, r->src, off, len};
    run_parallel((int64_t)n, host_threads(), batch_copy_range, &bj);
    if (n) memset(arena + pos, 0, KMP_ARENA_SLACK);
    if (used_bytes) *used_bytes = n ? pos + KMP_ARENA_SLACK : 0;
    return (int64_t)n;
}

/* openmp_task.c:130-137 with the extraction left to the device: record headers only. */
int64_t kmp_batch_next_frames(kmp_batch_reader *r, uint64_t max_span_bytes, uint64_t *frame_off, uint32_t *frame_caplen,
                              uint64_t cap_frames)
{
    if (!r || !frame_off || !frame_caplen || cap_frames == 0) return KMPHOST_EINVAL;
    uint64_t n = 0, first = 0;
    while (!r->eof && n < cap_frames) {
        const uint64_t before = r->walk.pos;
        uint32_t cl, ln;
        const uint8_t *data;
        if (walk_next(&r->walk, &cl, &ln, &data) < 0) { r->eof = 1; break; }                  /* openmp_task.c:135 */
        const uint64_t o = (uint64_t)(data - r->view.base);
        if (n == 0) first = o;
        else if (o + cl - first > max_span_bytes) { r->walk.pos = before; break; }           /* this record opens the next batch */
        frame_off[n] = o; frame_caplen[n] = cl; n++;
    }
    return (int64_t)n;
}

const uint8_t *kmp_batch_file(const kmp_batch_reader *r, uint64_t *nbytes)
{
    if (nbytes) *nbytes = r ? r->view.size : 0;
    return r ? r->view.base : NULL;
}

/* One piece of kmp_copy_bytes.  The destination is a pinned staging buffer that the GPU's copy engine reads next and the CPU never
 * reads again: streaming (non-temporal) stores write it past the caches -- no read-for-ownership of the destination lines, and the
 * DMA that follows finds the bytes in DRAM instead of probing dirty lines out of sixteen cores' caches. */
static void copy_streaming(uint8_t *dst, const uint8_t *src, uint64_t n)
{
#if defined(__SSE2__)
    uint64_t head = (16u - ((uintptr_t)dst & 15u)) & 15u;
    if (head > n) head = n;
    if (head) { memcpy(dst, src, (size_t)head); dst += head; src += head; n -= head; }
    const uint64_t body = n & ~(uint64_t)63;
    for (uint64_t o = 0; o < body; o += 64) {
        const __m128i a = _mm_loadu_si128((const __m128i *)(src + o)), b = _mm_loadu_si128((const __m128i *)(src + o + 16));
        const __m128i c = _mm_loadu_si128((const __m128i *)(src + o + 32)), d = _mm_loadu_si128((const __m128i *)(src + o + 48));
        _mm_stream_si128((__m128i *)(dst + o), a); _mm_stream_si128((__m128i *)(dst + o + 16), b);
        _mm_stream_si128((__m128i *)(dst + o + 32), c); _mm_stream_si128((__m128i *)(dst + o + 48), d);
    }
    if (n > body) memcpy(dst + body, src + body, (size_t)(n - body));
    _mm_sfence();
#else
    memcpy(dst, src, (size_t)n);
#endif
}

typedef struct bytes_copy_job { uint8_t *dst; const uint8_t *src; uint64_t n, piece; } bytes_copy_job;
static void bytes_copy_range(void *arg, int64_t lo, int64_t hi)
{
    const bytes_copy_job *j = (const bytes_copy_job *)arg;
    for (int64_t i = lo; i < hi; i++) {
        const uint64_t o = (uint64_t)i * j->piece, l = (j->n - o < j->piece) ? j->n - o : j->piece;
        copy_streaming(j->dst + o, j->src + o, l);
    }
}

void kmp_copy_bytes(uint8_t *dst, const uint8_t *src, uint64_t n)
{
    const uint64_t piece = 1u << 20;
    bytes_copy_job bj = {dst, src, n, piece};
    run_parallel((int64_t)((n + piece - 1) / piece), host_threads(), bytes_copy_range, &bj);
}

void kmp_batch_close(kmp_batch_reader *r)
{
    if (!r) return;
    view_close(&r->view);
    free(r->src);
    free(r);
}

/* ============================ synthetic payloads ======================================== */

void kmp_synth_fill_host(uint8_t *arena, const uint64_t *off, const uint32_t *len, uint64_t first_pkt_id,
                         uint64_t n, const kmp_synth_params *sp, int threads)
{
    if (threads < 1) threads = 1;
    (void)threads;
#pragma omp parallel for num_threads(threads) schedule(static)
    for (int64_t i = 0; i < (int64_t)n; i++) {
        const uint64_t id = first_pkt_id + (uint64_t)i;
        const uint32_t L = len[i];
        const uint32_t key = kmp_synth_pkt_key(sp->seed, id);
        uint32_t pos = 0;
        const int planted = kmp_synth_plant(sp, id, L, &pos);
        uint32_t *slot = (uint32_t *)(arena + off[i]);
        const uint32_t nw = ((L + 15u) & ~15u) / 4u;
        for (uint32_t w = 0; w < nw; w++) slot[w] = kmp_synth_slot_word(sp, key, w, L, planted, pos);
    }
}

uint64_t kmp_synth_count_planted(const uint32_t *len, uint32_t fixed_len, uint64_t first_pkt_id, uint64_t n,
                                 const kmp_synth_params *sp)
{
    uint64_t c = 0;
    for (uint64_t i = 0; i < n; i++) {
        uint32_t pos;
        c += (uint64_t)kmp_synth_plant(sp, first_pkt_id + i, len ? len[i] : fixed_len, &pos);
    }
    return c;
}

/* ============================ report ==================================================== */

/* serial.c:163-169 (the misspelling is the reference's). */
void kmp_report(FILE *fp, const kmp_patterns *pats, const uint64_t *counts, double elapsed_seconds)
{
    fprintf(fp, "Printing the number of appereances of each string throughout the entire pcap file:\n");
    for (uint32_t i = 0; i < pats->n; i++)
        if (counts[i] != 0) {
            /* The reference counts in int (serial.c:101) and prints %d (serial.c:166): beyond INT_MAX its own counter
             * has overflowed (undefined).  The line keeps the %d form -- the low 32 bits, as a wrapped int prints --
             * and the exact 64-bit count goes to stderr. */
            if (counts[i] > 2147483647ull)
                fprintf(stderr, "[kmphost] warning: %s matched %llu times, more than an int holds; the report line shows the wrapped value the reference's int counter would print\n",
                        (const char *)(pats->blob + pats->off[i]), (unsigned long long)counts[i]);
            fprintf(fp, "%s: %d times!\n", (const char *)(pats->blob + pats->off[i]), (int)counts[i]);
        }
    fprintf(fp, "Elapsed time = %f seconds\n", elapsed_seconds);
}

/* ============================ pcap writer (tooling) ===================================== */

/* append == 0: a new file, global header first; != 0: records behind what the file holds */
int kmp_write_udp_pcap_part(const char *path, int append, const uint8_t *arena, const uint64_t *off, const uint32_t *len, uint64_t n,
                            uint64_t first_record)
{
    FILE *fp = fopen(path, append ? "ab" : "wb");
    if (!fp) return KMPHOST_EIO;
    const uint32_t gh[6] = {0xA1B2C3D4u, 0x00040002u, 0, 0, 262144u, 1u};   /* v2.4, Ethernet */
    if (!append && fwrite(gh, sizeof gh, 1, fp) != 1) { fclose(fp); return KMPHOST_EIO; }
    uint8_t hdr[42];
    memset(hdr, 0, sizeof hdr);
    for (int i = 0; i < 12; i++) hdr[i] = (uint8_t)(i + 1);
    hdr[12] = 0x08; hdr[13] = 0x00;             /* IPv4 */
    hdr[14] = 0x45;                             /* version 4, IHL 5 */
    hdr[22] = 64;                               /* TTL */
    hdr[23] = 17;                               /* UDP */
    for (uint64_t k = 0; k < n; k++) {
        const uint64_t rec = first_record + k;
        const uint32_t L = len[k], tot = 42u + L;
        const uint32_t rh[4] = {(uint32_t)(rec / 1000000u), (uint32_t)(rec % 1000000u), tot, tot};
        hdr[16] = (uint8_t)((28u + L) >> 8); hdr[17] = (uint8_t)(28u + L);
        hdr[38] = (uint8_t)((8u + L) >> 8); hdr[39] = (uint8_t)(8u + L);
        if (fwrite(rh, sizeof rh, 1, fp) != 1 || fwrite(hdr, sizeof hdr, 1, fp) != 1 ||
            (L && fwrite(arena + off[k], L, 1, fp) != 1)) {
            fclose(fp);
            return KMPHOST_EIO;
        }
    }
    return fclose(fp) ? KMPHOST_EIO : KMPHOST_OK;
}

int kmp_write_udp_pcap(const char *path, const uint8_t *arena, const uint64_t *off, const uint32_t *len, uint64_t n)
{
    return kmp_write_udp_pcap_part(path, 0, arena, off, len, n, 0);
}
