/* Built with -fsanitize=address,undefined by tests/test_thresholds_host.py: drives the packer of the rate thresholds' tables
 * (csrc/kmp_rowtables.cpp, kmp_pack_thresholds), the parser of their file (csrc/host/kmphost.c, kmp_thresholds_parse) and the reader of a
 * capture's timestamps (kmp_arena_from_pcap_ts) without a device.  Every expected table and time below is written out by hand from the
 * descriptions in csrc/kmp_rowtables.h and include/kmphost.h, none is computed by the code under test.
 * argv[1]: a directory the files may be written to; argv[2]: tests/golden/data/tcp.pcap. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "kmp_rowtables.h"
#include "kmphost.h"

typedef std::vector<uint32_t> Words;
typedef std::vector<kmpgpu_threshold> Thr;

static int g_failed = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "CHECK failed: %s (line %d)\n", #c, __LINE__); g_failed++; } } while (0)

static const uint32_t BY_RULE = KMPGPU_THR_BY_RULE, BY_SRC = KMPGPU_THR_BY_SRC, BY_DST = KMPGPU_THR_BY_DST, BY_FLOW = KMPGPU_THR_BY_FLOW;
static const uint32_t AT_LEAST = KMPGPU_THR_AT_LEAST, AT_MOST = KMPGPU_THR_AT_MOST, EXACTLY = KMPGPU_THR_EXACTLY;
static const uint64_t ALL = KMPGPU_THR_NO_WINDOW;

static bool refused(const Thr &thr, uint32_t n_rules, const char *text)
{
    kmp_threshold_tables t;
    std::string msg;
    const int rc = kmp_pack_thresholds(thr.data(), (uint32_t)thr.size(), n_rules, &t, &msg);
    bool ok = rc == KMPGPU_EINVAL && msg == std::string("kmpgpu_set_thresholds: ") + text && t.final_table.empty() && !t.windowed;
    for (int x = 0; x < 4; x++) ok = ok && t.by_track[x].empty();
    if (!ok) fprintf(stderr, "rc %d, message '%s' (wanted 'kmpgpu_set_thresholds: %s')\n", rc, msg.c_str(), text);
    return ok;
}

static void packer(void)
{
    {
        kmp_threshold_tables t;
        std::string msg;
        CHECK(kmp_pack_thresholds(nullptr, 1, 1, &t, &msg) == KMPGPU_EINVAL && msg == "kmpgpu_set_thresholds: thr is NULL");
    }
    CHECK(refused({{0, BY_SRC, AT_LEAST, 1, 5}, {2, BY_SRC, AT_LEAST, 1, 5}}, 2, "threshold 1 names rule 2 of 2"));
    CHECK(refused({{0, 4, AT_LEAST, 1, 5}}, 1, "threshold 0: track 4 is none of KMPGPU_THR_BY_*"));
    CHECK(refused({{0, BY_FLOW, 3, 1, 5}}, 1, "threshold 0: type 3 is none of KMPGPU_THR_AT_LEAST, _AT_MOST, _EXACTLY"));
    CHECK(refused({{0, BY_RULE, EXACTLY, 0, 5}}, 1, "threshold 0: count is 0"));
    CHECK(refused({{0, BY_RULE, EXACTLY, 1, 5}, {0, BY_DST, AT_MOST, 1, 0}}, 1, "threshold 1: window is 0 (no payload lies inside it)"));

    /* four rules, thresholds out of rule order, two on rule 2, none on rule 1 */
    kmp_threshold_tables t;
    std::string msg;
    const Thr thr = {{2, BY_SRC, AT_LEAST, 5, 60000000}, {0, BY_FLOW, AT_MOST, 1, ALL}, {3, BY_RULE, EXACTLY, 2, 1}, {2, BY_RULE, AT_MOST, 9, ALL},
                     {0, BY_SRC, AT_LEAST, 0xFFFFFFFFu, 0xFFFFFFFFFFFFFFFEull}};
    CHECK(kmp_pack_thresholds(thr.data(), 5, 4, &t, &msg) == KMPGPU_OK && msg.empty());
    CHECK(t.by_track[BY_RULE] == Words({2, 3}) && t.by_track[BY_SRC] == Words({0, 4}) && t.by_track[BY_DST].empty() && t.by_track[BY_FLOW] == Words({1}));
    CHECK(t.windowed);
    /* {first, number} of rules 0..3, then the list: rule 0's 1, 4; rule 2's 0, 3; rule 3's 2 */
    CHECK(t.final_table == Words({0, 2, 2, 0, 2, 2, 4, 1, 1, 4, 0, 3, 2}));
    /* no window anywhere: the timestamps are not needed */
    CHECK(kmp_pack_thresholds(thr.data() + 1, 1, 1, &t, &msg) == KMPGPU_OK && !t.windowed && t.final_table == Words({0, 1, 0}));
}

/* ---- the file parser ---------------------------------------------------------------------------------------------------------------- */
static std::string g_dir;

static int parse_text(const char *text, uint32_t n_rules, kmp_thresholds *out, std::string *err)
{
    const std::string path = g_dir + "/thresholds.txt";
    FILE *fp = fopen(path.c_str(), "wb");
    if (!fp) { perror(path.c_str()); g_failed++; return -100; }
    fputs(text, fp);
    fclose(fp);
    char buf[KMP_THRESHOLDS_ERRBUF];
    memset(buf, 'x', sizeof buf);
    const int rc = kmp_thresholds_parse(path.c_str(), n_rules, out, buf);
    *err = buf;
    return rc;
}

static bool parse_refused(const char *text, uint32_t n_rules, const char *want)
{
    kmp_thresholds f;
    std::string err;
    const int rc = parse_text(text, n_rules, &f, &err);
    const bool ok = rc == KMPHOST_EINVAL && err == want && f.thr == nullptr && f.n == 0;
    if (!ok) fprintf(stderr, "rc %d, message '%s' (wanted '%s')\n", rc, err.c_str(), want);
    kmp_thresholds_free(&f);
    return ok;
}

static bool same(const kmp_threshold &a, const kmp_threshold &b)
{
    return a.rule == b.rule && a.track == b.track && a.type == b.type && a.count == b.count && a.window == b.window;
}

static void parser(void)
{
    kmp_thresholds f;
    std::string err;
    CHECK(parse_text("# the fifth failed login in a minute\n\n0 by_src at_least 5 60\n  1 by_dst at_most 1 0.5\n2\tby_flow   exactly 4294967295 all\n"
                     "0 by_rule at_most 2 0.000001\n1 by_rule at_least 1 18446744073709.551614\n2 by_src at_least 3 007.250000\n", 3, &f, &err) == KMPHOST_OK);
    CHECK(err.empty() && f.n == 6);
    const kmp_threshold want[6] = {{0, KMP_THR_BY_SRC, KMP_THR_AT_LEAST, 5, 60000000ull}, {1, KMP_THR_BY_DST, KMP_THR_AT_MOST, 1, 500000ull},
                                   {2, KMP_THR_BY_FLOW, KMP_THR_EXACTLY, 4294967295u, KMP_THR_NO_WINDOW}, {0, KMP_THR_BY_RULE, KMP_THR_AT_MOST, 2, 1ull},
                                   {1, KMP_THR_BY_RULE, KMP_THR_AT_LEAST, 1, 18446744073709551614ull}, {2, KMP_THR_BY_SRC, KMP_THR_AT_LEAST, 3, 7250000ull}};
    for (uint32_t q = 0; q < 6 && q < f.n; q++) CHECK(same(f.thr[q], want[q]));
    /* what the parser gives is what the packer takes */
    kmp_threshold_tables t;
    std::string msg;
    CHECK(kmp_pack_thresholds((const kmpgpu_threshold *)f.thr, f.n, 3, &t, &msg) == KMPGPU_OK && t.by_track[BY_SRC] == Words({0, 5}));
    kmp_thresholds_free(&f);
    CHECK(f.thr == nullptr && f.n == 0);
    /* an empty file: no thresholds */
    CHECK(parse_text("# nothing\n", 1, &f, &err) == KMPHOST_OK && f.n == 0 && f.thr == nullptr);
    kmp_thresholds_free(&f);
    /* more lines than the first allocation holds */
    std::string many;
    for (int i = 0; i < 100; i++) many += "0 by_rule at_least " + std::to_string(i + 1) + " 1\n";
    CHECK(parse_text(many.c_str(), 1, &f, &err) == KMPHOST_OK && f.n == 100 && f.thr[99].count == 100);
    kmp_thresholds_free(&f);

    CHECK(parse_refused("0 by_src at_least 5 60\n\nx by_src at_least 5 60\n", 1, "line 3: 'x' is not a rule index"));
    CHECK(parse_refused("-1 by_src at_least 5 60\n", 1, "line 1: '-1' is not a rule index"));
    CHECK(parse_refused("# c\n1 by_src at_least 5 60\n", 1, "line 2: rule 1 of 1"));
    CHECK(parse_refused("0\n", 1, "line 1: rule 0 has no track (by_rule, by_src, by_dst, by_flow)"));
    CHECK(parse_refused("0 by_pair at_least 5 60\n", 1, "line 1: 'by_pair' is none of by_rule by_src by_dst by_flow"));
    CHECK(parse_refused("0 by_src\n", 1, "line 1: rule 0 has no type (at_least, at_most, exactly)"));
    CHECK(parse_refused("0 by_src both 5 60\n", 1, "line 1: 'both' is none of at_least at_most exactly"));
    CHECK(parse_refused("0 by_src at_least\n", 1, "line 1: rule 0 has no count"));
    CHECK(parse_refused("0 by_src at_least 0 60\n", 1, "line 1: '0' is not a count in 1..4294967295"));
    CHECK(parse_refused("0 by_src at_least 4294967296 60\n", 1, "line 1: '4294967296' is not a count in 1..4294967295"));
    CHECK(parse_refused("0 by_src at_least five 60\n", 1, "line 1: 'five' is not a count in 1..4294967295"));
    CHECK(parse_refused("0 by_src at_least 5\n", 1, "line 1: rule 0 has no window (seconds, or all)"));
    CHECK(parse_refused("0 by_src at_least 5 60s\n", 1, "line 1: '60s' is neither all nor seconds with at most 6 fraction digits"));
    CHECK(parse_refused("0 by_src at_least 5 .5\n", 1, "line 1: '.5' is neither all nor seconds with at most 6 fraction digits"));
    CHECK(parse_refused("0 by_src at_least 5 1.\n", 1, "line 1: '1.' is neither all nor seconds with at most 6 fraction digits"));
    CHECK(parse_refused("0 by_src at_least 5 0.0000001\n", 1, "line 1: '0.0000001' is neither all nor seconds with at most 6 fraction digits"));
    CHECK(parse_refused("0 by_src at_least 5 1.5.2\n", 1, "line 1: '1.5.2' is neither all nor seconds with at most 6 fraction digits"));
    CHECK(parse_refused("0 by_src at_least 5 -1\n", 1, "line 1: '-1' is neither all nor seconds with at most 6 fraction digits"));
    CHECK(parse_refused("0 by_src at_least 5 18446744073709.551615\n", 1, "line 1: '18446744073709.551615' seconds are more than 2^64 - 2 microseconds"));
    CHECK(parse_refused("0 by_src at_least 5 99999999999999999999999\n", 1, "line 1: '99999999999999999999999' seconds are more than 2^64 - 2 microseconds"));
    CHECK(parse_refused("0 by_src at_least 5 0\n", 1, "line 1: '0': a window of 0 holds no payload"));
    CHECK(parse_refused("0 by_src at_least 5 0.000000\n", 1, "line 1: '0.000000': a window of 0 holds no payload"));
    CHECK(parse_refused("0 by_src at_least 5 60 seconds\n", 1, "line 1: 'seconds' follows the window"));
    {
        char buf[KMP_THRESHOLDS_ERRBUF];
        CHECK(kmp_thresholds_parse((g_dir + "/no such file").c_str(), 1, &f, buf) == KMPHOST_EIO && f.thr == nullptr);
    }
}

/* ---- the capture's timestamps ------------------------------------------------------------------------------------------------------- */
static void put32(std::string *s, uint32_t v, bool big)
{
    for (int i = 0; i < 4; i++) s->push_back((char)(v >> (big ? 24 - 8 * i : 8 * i)));
}

/* an Ethernet + IPv4 + UDP frame with a payload of `len` bytes 'p' */
static std::string udp_frame(uint32_t len, uint8_t proto)
{
    std::string f(14 + 20 + 8, '\0');
    f[12] = 0x08; f[14] = 0x45; f[23] = (char)proto;
    f[26] = 10; f[29] = 1; f[30] = 10; f[33] = 2;
    return f + std::string(len, 'p');
}

/* a classic capture of the given magic in the given byte order: records (sec, frac, frame) */
struct Rec { uint32_t sec, frac; std::string frame; };
static std::string classic(uint32_t magic, bool big, const std::vector<Rec> &recs)
{
    std::string s;
    put32(&s, magic, big);
    s += big ? std::string("\0\2\0\4", 4) : std::string("\2\0\4\0", 4);
    put32(&s, 0, big); put32(&s, 0, big); put32(&s, 65535, big); put32(&s, 1, big);
    for (const Rec &r : recs) {
        put32(&s, r.sec, big); put32(&s, r.frac, big); put32(&s, (uint32_t)r.frame.size(), big); put32(&s, (uint32_t)r.frame.size(), big);
        s += r.frame;
    }
    return s;
}

/* a pcapng section: header, one interface, Enhanced Packet Blocks with (hi, lo) timestamps and one Simple Packet Block in the middle.
 * trailer: what stands in every packet block's trailing length word instead of its length (0: the length) -- the walker checks the leading
 * word alone, so such a file is read, and nothing may be looked up through the trailing one */
static std::string pcapng(const std::vector<Rec> &recs, uint32_t trailer = 0)
{
    std::string s;
    put32(&s, 0x0A0D0D0Au, false); put32(&s, 28, false); put32(&s, 0x1A2B3C4Du, false); put32(&s, 1, false);      /* (version 1.0 as two halves) */
    put32(&s, 0xFFFFFFFFu, false); put32(&s, 0xFFFFFFFFu, false); put32(&s, 28, false);
    put32(&s, 1, false); put32(&s, 20, false); put32(&s, 1, false); put32(&s, 65535, false); put32(&s, 20, false);
    for (size_t i = 0; i < recs.size(); i++) {
        const Rec &r = recs[i];
        const uint32_t cl = (uint32_t)r.frame.size(), pad = (4u - cl % 4u) % 4u;
        if (i == 1) {                               /* a Simple Packet Block: no time */
            put32(&s, 3, false); put32(&s, 16 + cl + pad, false); put32(&s, cl, false);
            s += r.frame + std::string(pad, '\0');
            put32(&s, trailer ? trailer : 16 + cl + pad, false);
            continue;
        }
        put32(&s, 6, false); put32(&s, 32 + cl + pad, false); put32(&s, 0, false); put32(&s, r.sec, false); put32(&s, r.frac, false);
        put32(&s, cl, false); put32(&s, cl, false);
        s += r.frame + std::string(pad, '\0');
        put32(&s, trailer ? trailer : 32 + cl + pad, false);
    }
    return s;
}

static bool times_of(const std::string &bytes, int proto, const std::vector<uint64_t> &want, bool with_meta)
{
    const std::string path = g_dir + "/capture.pcap";
    FILE *fp = fopen(path.c_str(), "wb");
    if (!fp) { perror(path.c_str()); return false; }
    fwrite(bytes.data(), 1, bytes.size(), fp);
    fclose(fp);
    kmp_arena a;
    kmp_pkt_meta *meta = nullptr;
    uint64_t *ts = nullptr;
    char err[KMP_PCAP_ERRBUF];
    const int rc = kmp_arena_from_pcap_ts(path.c_str(), proto, nullptr, nullptr, &a, err, with_meta ? &meta : nullptr, &ts);
    bool ok = rc == KMPHOST_OK && a.n_pkts == want.size() && ts != nullptr && (meta != nullptr) == with_meta;
    for (size_t k = 0; ok && k < want.size(); k++) {
        ok = ts[k] == want[k];
        if (!ok) fprintf(stderr, "payload %zu: %llu, wanted %llu\n", k, (unsigned long long)ts[k], (unsigned long long)want[k]);
    }
    if (!ok) fprintf(stderr, "rc %d, %llu payloads (wanted %zu)\n", rc, (unsigned long long)a.n_pkts, want.size());
    /* the arena is the one of kmp_arena_from_pcap */
    kmp_arena b;
    ok = ok && kmp_arena_from_pcap(path.c_str(), proto, nullptr, nullptr, &b, err) == KMPHOST_OK && b.n_pkts == a.n_pkts && b.nbytes == a.nbytes &&
         !memcmp(a.bytes, b.bytes, (size_t)a.nbytes) && !memcmp(a.off, b.off, (size_t)a.n_pkts * 8) && !memcmp(a.len, b.len, (size_t)a.n_pkts * 4);
    if (rc == KMPHOST_OK) { kmp_arena_free(&a); kmp_arena_free(&b); }
    free(meta);
    free(ts);
    return ok;
}

static void timestamps(const char *golden)
{
    /* four frames, the third one TCP: the udp extractor skips it, and its time with it */
    const std::vector<Rec> recs = {{1, 999999, udp_frame(5, 17)}, {2, 0, udp_frame(0, 17)}, {3, 7, udp_frame(9, 6)}, {0xFFFFFFFFu, 123456, udp_frame(33, 17)}};
    CHECK(times_of(classic(0xA1B2C3D4u, false, recs), KMP_PROTO_UDP, {1999999ull, 2000000ull, 4294967295123456ull}, true));
    CHECK(times_of(classic(0xA1B2C3D4u, true, recs), KMP_PROTO_UDP, {1999999ull, 2000000ull, 4294967295123456ull}, false));
    /* the nanosecond magic: ts_frac / 1000, rounded down */
    const std::vector<Rec> nano = {{1, 999999999, udp_frame(5, 17)}, {2, 999, udp_frame(0, 17)}, {3, 7, udp_frame(9, 6)}, {4, 1000, udp_frame(33, 17)}};
    CHECK(times_of(classic(0xA1B23C4Du, false, nano), KMP_PROTO_UDP, {1999999ull, 2000000ull, 4000001ull}, true));
    CHECK(times_of(classic(0xA1B23C4Du, true, nano), KMP_PROTO_UDP, {1999999ull, 2000000ull, 4000001ull}, false));
    /* pcapng: the two halves as one 64-bit number of microseconds; a Simple Packet Block has none */
    CHECK(times_of(pcapng({{5, 6, udp_frame(5, 17)}, {0, 0, udp_frame(2, 17)}, {0xFFFFFFFFu, 0xFFFFFFFEu, udp_frame(7, 17)}}), KMP_PROTO_UDP,
                   {5ull << 32 | 6ull, 0ull, 0xFFFFFFFFFFFFFFFEull}, true));
    /* trailing length words that do not match: far outside the file, in front of it, 0 -- the same times */
    for (const uint32_t trailer : {0xFFFFFFFCu, 0x7FFFFFF0u, 4u, 1u << 20})
        CHECK(times_of(pcapng({{5, 6, udp_frame(5, 17)}, {0, 0, udp_frame(2, 17)}, {0xFFFFFFFFu, 0xFFFFFFFEu, udp_frame(7, 17)}}, trailer), KMP_PROTO_UDP,
                       {5ull << 32 | 6ull, 0ull, 0xFFFFFFFFFFFFFFFEull}, false));
    /* no frames, and ts_out NULL */
    CHECK(times_of(classic(0xA1B2C3D4u, false, {}), KMP_PROTO_UDP, {}, true));
    {
        kmp_arena a;
        char err[KMP_PCAP_ERRBUF];
        CHECK(kmp_arena_from_pcap_ts(golden, KMP_PROTO_TCP, nullptr, nullptr, &a, err, nullptr, nullptr) == KMPHOST_OK && a.n_pkts == 13);
        kmp_arena_free(&a);
        uint64_t *ts = (uint64_t *)1;
        CHECK(kmp_arena_from_pcap_ts((g_dir + "/no such file").c_str(), KMP_PROTO_TCP, nullptr, nullptr, &a, err, nullptr, &ts) == KMPHOST_EIO && ts == nullptr);
    }
    /* the fixture: 13 TCP segments; the first, the first GET and the last as a hex dump of the file shows them */
    {
        kmp_arena a;
        kmp_pkt_meta *meta = nullptr;
        uint64_t *ts = nullptr;
        char err[KMP_PCAP_ERRBUF];
        CHECK(kmp_arena_from_pcap_ts(golden, KMP_PROTO_TCP, nullptr, nullptr, &a, err, &meta, &ts) == KMPHOST_OK && a.n_pkts == 13 && ts && meta);
        if (ts && a.n_pkts == 13) {
            CHECK(ts[0] == 1607111499289993ull && ts[3] == 1607111499418127ull && ts[12] == 1607111501325078ull);
            for (int k = 1; k < 13; k++) CHECK(ts[k] >= ts[k - 1]);
        }
        kmp_arena_free(&a);
        free(meta);
        free(ts);
        /* ... and with the sequence numbers beside them, which are those of kmp_arena_from_pcap_seq */
        uint32_t *seq = nullptr, *seq2 = nullptr;
        kmp_arena b;
        ts = nullptr;
        CHECK(kmp_arena_from_pcap_seq_ts(golden, KMP_PROTO_TCP, nullptr, nullptr, &a, err, nullptr, &seq, &ts) == KMPHOST_OK && seq && ts);
        CHECK(kmp_arena_from_pcap_seq(golden, KMP_PROTO_TCP, nullptr, nullptr, &b, err, nullptr, &seq2) == KMPHOST_OK && seq2);
        if (seq && seq2 && ts) CHECK(a.n_pkts == 13 && b.n_pkts == 13 && !memcmp(seq, seq2, 13 * sizeof(uint32_t)) && ts[12] == 1607111501325078ull);
        kmp_arena_free(&a);
        kmp_arena_free(&b);
        free(seq); free(seq2); free(ts);
    }
}

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s <directory> <tcp.pcap>\n", argv[0]); return 2; }
    g_dir = argv[1];
    packer();
    parser();
    timestamps(argv[2]);
    if (g_failed) { fprintf(stderr, "%d checks failed\n", g_failed); return 1; }
    printf("thresholds driver ok\n");
    return 0;
}
