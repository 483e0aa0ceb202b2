/* Built with -fsanitize=address,undefined by tests/test_bytetests_host.py: drives kmp_pack_bytetests and the n_bt entries of the rules,
 * relations, chains and headers packers (csrc/kmp_rowtables.cpp), and kmp_bytetests_parse / kmp_rules_parse_bt (csrc/host/kmphost.c) on the
 * files named on the command line, without a device.  Every expected table below is written out by hand from the description of the
 * device form in csrc/kmp_rowtables.h, none is computed by the code under test.
 *   argv[1]: a byte tests file that parses (3 patterns), argv[2]: one that does not, argv[3]: a rules file with b<q> terms */
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "kmp_rowtables.h"
#include "kmphost.h"

typedef std::vector<uint32_t> Words;

static int g_failed = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "CHECK failed: %s (line %d)\n", #c, __LINE__); g_failed++; } } while (0)

static const uint32_t N = KMPGPU_RULE_NOT;

static bool refused(int rc, const std::string &msg, const char *text)
{
    const bool ok = rc == KMPGPU_EINVAL && msg == text;
    if (!ok) fprintf(stderr, "rc %d, message '%s' (wanted '%s')\n", rc, msg.c_str(), text);
    return ok;
}

static kmpgpu_bytetest test(uint32_t anchor, int32_t offset, uint32_t mask, uint32_t value, uint8_t nbytes, uint8_t op, uint8_t flags)
{
    kmpgpu_bytetest b;
    memset(&b, 0, sizeof b);
    b.anchor = anchor; b.offset = offset; b.mask = mask; b.value = value; b.nbytes = nbytes; b.op = op; b.flags = flags;
    return b;
}

static void bytetests(void)
{
    /* patterns 0 .. 2, pattern 1 of the nocase set */
    const uint8_t fold[3] = {0, 1, 0};
    const std::vector<kmpgpu_bytetest> t = {
        test(0, 2, 0x8000u, 0, 2, KMPGPU_BT_NE, 0),                                   /* the QR bit of a DNS message */
        test(1, -3, 0xFFFFFFFFu, 512, 2, KMPGPU_BT_GT, KMPGPU_BT_RELATIVE),            /* behind a nocase anchor: bit 31 */
        test(0, 0x7FFFFFFF, 0, 0xFFFFFFFFu, 4, KMPGPU_BT_GE, KMPGPU_BT_LITTLE),        /* the largest offset */
        test(2, 0, 0xFFu, 7, 1, KMPGPU_BT_LE, KMPGPU_BT_RELATIVE | KMPGPU_BT_LITTLE),
        test(0, 9, 0xFFFFFFFFu, 0, 3, KMPGPU_BT_EQ, 0),
    };
    const Words want = {
        0, 2, 0x8000u, 0,                          2u | 1u << 8, 0, 0, 0,
        0x80000001u, 0xFFFFFFFDu, 0xFFFFFFFFu, 512, 2u | 3u << 8 | 1u << 16, 0, 0, 0,
        0, 0x7FFFFFFFu, 0, 0xFFFFFFFFu,             4u | 5u << 8 | 2u << 16, 0, 0, 0,
        2, 0, 0xFFu, 7,                             1u | 4u << 8 | 3u << 16, 0, 0, 0,
        0, 9, 0xFFFFFFFFu, 0,                       3u, 0, 0, 0,
        1, 3,                                       /* the relative tests, ascending */
    };
    Words got;
    std::string msg;
    uint32_t n_rel = 77, reach = 77;
    CHECK(kmp_pack_bytetests(t.data(), 5, 3, 1, 1, 2, fold, &got, &n_rel, &reach, &msg) == KMPGPU_OK);
    CHECK(got == want && n_rel == 2 && reach == 0x80000003u);
    /* without the far test the reach is the largest offset + nbytes of the absolute ones: 9 + 3 */
    std::vector<kmpgpu_bytetest> b = t;
    b[2].offset = 1;
    CHECK(kmp_pack_bytetests(b.data(), 5, 3, 0, 0, 0, fold, &got, &n_rel, &reach, &msg) == KMPGPU_OK && reach == 12 && n_rel == 2);
    /* relative tests alone: no reach */
    CHECK(kmp_pack_bytetests(&t[1], 1, 3, 0, 0, 0, fold, &got, &n_rel, &reach, &msg) == KMPGPU_OK && reach == 0 && n_rel == 1 && got.size() == 9 && got[8] == 0);

    /* every refusal; the table comes back empty */
    CHECK(refused(kmp_pack_bytetests(nullptr, 1, 3, 0, 0, 0, fold, &got, &n_rel, &reach, &msg), msg, "kmpgpu_set_bytetests: bt is NULL"));
    CHECK(got.empty() && n_rel == 0 && reach == 0);
    b = t; b[1].nbytes = 0;
    CHECK(refused(kmp_pack_bytetests(b.data(), 5, 3, 0, 0, 0, fold, &got, &n_rel, &reach, &msg), msg, "kmpgpu_set_bytetests: test 1 reads 0 bytes, not 1 .. 4"));
    b = t; b[4].nbytes = 5;
    CHECK(refused(kmp_pack_bytetests(b.data(), 5, 3, 0, 0, 0, fold, &got, &n_rel, &reach, &msg), msg, "kmpgpu_set_bytetests: test 4 reads 5 bytes, not 1 .. 4"));
    b = t; b[0].op = 6;
    CHECK(refused(kmp_pack_bytetests(b.data(), 5, 3, 0, 0, 0, fold, &got, &n_rel, &reach, &msg), msg, "kmpgpu_set_bytetests: test 0: unknown operator 6"));
    b = t; b[3].flags = 7;
    CHECK(refused(kmp_pack_bytetests(b.data(), 5, 3, 0, 0, 0, fold, &got, &n_rel, &reach, &msg), msg, "kmpgpu_set_bytetests: test 3: unknown flag bits 0x4"));
    b = t; b[2].reserved = 1;
    CHECK(refused(kmp_pack_bytetests(b.data(), 5, 3, 0, 0, 0, fold, &got, &n_rel, &reach, &msg), msg, "kmpgpu_set_bytetests: test 2: reserved is 1, not 0"));
    b = t; b[3].anchor = 3;
    CHECK(refused(kmp_pack_bytetests(b.data(), 5, 3, 0, 0, 0, fold, &got, &n_rel, &reach, &msg), msg, "kmpgpu_set_bytetests: test 3 names pattern 3 of 3"));
    b = t; b[0].anchor = 1;
    CHECK(refused(kmp_pack_bytetests(b.data(), 5, 3, 0, 0, 0, fold, &got, &n_rel, &reach, &msg), msg, "kmpgpu_set_bytetests: test 0 is absolute and names anchor 1, not 0"));
    b = t; b[4].offset = -1;
    CHECK(refused(kmp_pack_bytetests(b.data(), 5, 3, 0, 0, 0, fold, &got, &n_rel, &reach, &msg), msg,
                  "kmpgpu_set_bytetests: test 4 is absolute and its offset -1 lies in front of the payload"));
    CHECK(got.empty());

    /* the 2^31 bound is checked on the counts alone, before the array is read: one valid test stands for 2^31 - 14 of them */
    CHECK(refused(kmp_pack_bytetests(t.data(), 0x7FFFFFF2u, 8, 2, 1, 3, fold, &got, &n_rel, &reach, &msg), msg,
                  "kmpgpu_set_bytetests: 8 patterns + 2 relations + 1 chains + 3 header predicates + 2147483634 byte tests do not fit the 2^31 rows a rule term can name"));
    /* one below it passes the bound (5 tests, 2^31 - 6 patterns: 2^31 - 1 rows) */
    const std::vector<uint8_t> wide(4, 0);
    CHECK(kmp_pack_bytetests(t.data(), 5, 0x7FFFFFFAu, 0, 0, 0, wide.data(), &got, &n_rel, &reach, &msg) == KMPGPU_OK && got.size() == 42);
}

/* the n_bt entries of the other packers: the rules' terms reach the tests' rows, every 2^31 bound counts them in, and the entries without
 * n_bt are the ones with 0 */
static void siblings(void)
{
    /* 8 patterns + 1 relation + 1 chain + 2 predicates + 2 byte tests = rows 0 .. 13 */
    const Words off = {0, 2, 3}, terms = {12, N | 13, N | 12};
    const Words want_heads = {0, 0, 12, N | 13,  0, 0, N | 12, N | 12};
    Words heads, quads;
    std::string msg;
    CHECK(kmp_pack_rules(off.data(), terms.data(), 2, 8, 1, 1, 2, 2, &heads, &quads, &msg) == KMPGPU_OK);
    CHECK(heads == want_heads && quads.empty());
    CHECK(refused(kmp_pack_rules(off.data(), terms.data(), 2, 8, 1, 1, 2, 1, &heads, &quads, &msg), msg,
                  "kmpgpu_set_rules: rule 0: term 1 names row 13 of 8 patterns + 1 relations + 1 chains + 2 header predicates + 1 byte tests"));
    /* without n_bt a test's row is no row, and the messages are the ones they always were */
    CHECK(refused(kmp_pack_rules(off.data(), terms.data(), 2, 8, 1, 1, 2, &heads, &quads, &msg), msg,
                  "kmpgpu_set_rules: rule 0: term 0 names row 12 of 8 patterns + 1 relations + 1 chains + 2 header predicates"));
    CHECK(refused(kmp_pack_rules(off.data(), terms.data(), 2, 8, 1, 1, 2, 0, &heads, &quads, &msg), msg,
                  "kmpgpu_set_rules: rule 0: term 0 names row 12 of 8 patterns + 1 relations + 1 chains + 2 header predicates"));
    CHECK(refused(kmp_pack_rules(off.data(), terms.data(), 2, 8, 1, 1, &heads, &quads, &msg), msg,
                  "kmpgpu_set_rules: rule 0: term 0 names row 12 of 8 patterns + 1 relations + 1 chains"));

    const uint8_t fold[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const kmpgpu_relation rel = {1, 2, -3, 4};
    Words r;
    CHECK(kmp_pack_relations(&rel, 1, 8, 1, 5, 6, fold, &r, &msg) == KMPGPU_OK && r == Words({1, 2, 0xFFFFFFFDu, 4}));
    CHECK(refused(kmp_pack_relations(&rel, 1, 8, 0, 0, 0x7FFFFFF7u, fold, &r, &msg), msg,
                  "kmpgpu_set_relations: 8 patterns + 1 relations + the byte tests do not fit the 2^31 rows a rule term can name"));
    CHECK(refused(kmp_pack_relations(&rel, 1, 8, 1, 1, 0x7FFFFFF5u, fold, &r, &msg), msg,
                  "kmpgpu_set_relations: 8 patterns + 1 relations + the chains + the header predicates + the byte tests do not fit the 2^31 rows a rule term can name"));
    CHECK(kmp_pack_relations(&rel, 1, 8, 0, 0, 0x7FFFFFF6u, fold, &r, &msg) == KMPGPU_OK);
    CHECK(refused(kmp_pack_relations(&rel, 1, 8, 0, 0x7FFFFFF7u, fold, &r, &msg), msg,
                  "kmpgpu_set_relations: 8 patterns + 1 relations + the header predicates do not fit the 2^31 rows a rule term can name"));

    const Words coff = {0, 2};
    const kmpgpu_chain_link links[2] = {{1, INT32_MIN, INT32_MAX}, {2, 0, 5}};
    Words c;
    CHECK(kmp_pack_chains(coff.data(), links, 1, 8, 1, 3, 4, fold, &c, &msg) == KMPGPU_OK && c.size() == 4u * KMPGPU_CHAIN_MAX);
    CHECK(refused(kmp_pack_chains(coff.data(), links, 1, 8, 1, 0, 0x7FFFFFF6u, fold, &c, &msg), msg,
                  "kmpgpu_set_chains: 8 patterns + 1 relations + 1 chains + the byte tests do not fit the 2^31 rows a rule term can name"));
    CHECK(kmp_pack_chains(coff.data(), links, 1, 8, 1, 0, 0x7FFFFFF5u, fold, &c, &msg) == KMPGPU_OK);
    CHECK(refused(kmp_pack_chains(coff.data(), links, 1, 8, 1, 0x7FFFFFF6u, fold, &c, &msg), msg,
                  "kmpgpu_set_chains: 8 patterns + 1 relations + 1 chains + the header predicates do not fit the 2^31 rows a rule term can name"));

    kmpgpu_header h;
    memset(&h, 0, sizeof h);
    h.sport_hi = h.dport_hi = 0xFFFFu; h.len_hi = 0xFFFFFFFFu; h.flags = KMPGPU_HDR_ANY_PROTO;
    Words hw;
    CHECK(kmp_pack_headers(&h, 1, 8, 1, 1, 9, &hw, &msg) == KMPGPU_OK && hw.size() == 12);
    CHECK(refused(kmp_pack_headers(&h, 1, 8, 2, 1, 0x7FFFFFF4u, &hw, &msg), msg,
                  "kmpgpu_set_headers: 8 patterns + 2 relations + 1 chains + 1 header predicates + the byte tests do not fit the 2^31 rows a rule term can name"));
    CHECK(kmp_pack_headers(&h, 1, 8, 2, 1, 0x7FFFFFF3u, &hw, &msg) == KMPGPU_OK);
    CHECK(refused(kmp_pack_headers(&h, 0x7FFFFFF5u, 8, 2, 1, &hw, &msg), msg,
                  "kmpgpu_set_headers: 8 patterns + 2 relations + 1 chains + 2147483637 header predicates do not fit the 2^31 rows a rule term can name"));
}

/* the parsers on real files: what they allocate, grow and free */
static void parsers(const char *good, const char *bad, const char *rules)
{
    char err[KMP_BYTETESTS_ERRBUF];
    kmp_bytetests b;
    CHECK(kmp_bytetests_parse(good, 3, &b, err) == KMPHOST_OK && err[0] == 0);
    CHECK(b.n >= 100 && b.bt != nullptr);                 /* past the first allocation of 64 */
    if (b.n) {
        CHECK(b.bt[0].nbytes == 2 && b.bt[0].op == KMP_BT_NE && b.bt[0].mask == 0x8000u && b.bt[0].value == 0 && b.bt[0].offset == 2 && b.bt[0].flags == 0);
        /* what the parser leaves is what the packer takes */
        const uint8_t fold[3] = {0, 0, 0};
        Words got;
        std::string msg;
        uint32_t n_rel = 0, reach = 0;
        CHECK(kmp_pack_bytetests(reinterpret_cast<const kmpgpu_bytetest *>(b.bt), b.n, 3, 0, 0, 0, fold, &got, &n_rel, &reach, &msg) == KMPGPU_OK);
        CHECK(got.size() == 8u * b.n + n_rel);
    }
    const uint32_t n_bt = b.n;
    kmp_bytetests_free(&b);
    CHECK(b.n == 0 && b.bt == nullptr);
    kmp_bytetests_free(&b);                              /* twice, and NULL */
    kmp_bytetests_free(nullptr);

    CHECK(kmp_bytetests_parse(bad, 3, &b, err) == KMPHOST_EINVAL && strncmp(err, "line ", 5) == 0);
    CHECK(b.n == 0 && b.bt == nullptr);
    CHECK(kmp_bytetests_parse("/nonexistent/bytetests.txt", 3, &b, err) == KMPHOST_EIO && b.bt == nullptr);

    kmp_rules r;
    char rerr[KMP_RULES_ERRBUF];
    CHECK(kmp_rules_parse_bt(rules, 3, 0, 0, 0, n_bt, &r, rerr) == KMPHOST_OK && r.n >= 1);
    if (r.n) CHECK(r.terms[0] == 3u + n_bt - 1u);          /* its first term is the last test */
    kmp_rules_free(&r);
    /* the same file with no byte tests: "b<q>" is no term */
    CHECK(kmp_rules_parse_bt(rules, 3, 0, 0, 0, 0, &r, rerr) == KMPHOST_EINVAL && r.off == nullptr && r.terms == nullptr);
}

int main(int argc, char **argv)
{
    if (argc != 4) { fprintf(stderr, "usage: %s <good byte tests> <bad byte tests> <rules>\n", argv[0]); return 2; }
    bytetests();
    siblings();
    parsers(argv[1], argv[2], argv[3]);
    if (g_failed) { fprintf(stderr, "%d checks failed\n", g_failed); return 1; }
    printf("bytetests driver ok\n");
    return 0;
}
