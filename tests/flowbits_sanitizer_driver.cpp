/* Built with -fsanitize=address,undefined by tests/test_flowbits_host.py: drives the packer of the flow bits' tables
 * (csrc/kmp_rowtables.cpp, kmp_pack_flowbits) and the parser of their file (csrc/host/kmphost.c, kmp_flowbits_parse) without a device.
 * Every expected table and level below is written out by hand from the descriptions in csrc/kmp_rowtables.h and include/kmphost.h, none
 * is computed by the code under test.  argv[1]: a directory the files may be written to. */
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "kmp_rowtables.h"
#include "kmphost.h"

typedef std::vector<uint32_t> Words;
typedef std::vector<kmpgpu_flowbit_op> Ops;

static int g_failed = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "CHECK failed: %s (line %d)\n", #c, __LINE__); g_failed++; } } while (0)

static const uint32_t ISSET = KMPGPU_FB_ISSET, ISNOTSET = KMPGPU_FB_ISNOTSET, SET = KMPGPU_FB_SET, UNSET = KMPGPU_FB_UNSET,
                      TOGGLE = KMPGPU_FB_TOGGLE, NOALERT = KMPGPU_FB_NOALERT;
static const uint32_t ID0 = 0u, ID1 = 0xFFFFFFFFu;             /* the identity function's two masks */

static bool refused(const Ops &ops, uint32_t n_bits, uint32_t n_rules, const char *text)
{
    kmp_flowbit_tables t;
    std::string msg;
    const int rc = kmp_pack_flowbits(ops.data(), (uint32_t)ops.size(), n_bits, n_rules, &t, &msg);
    const bool ok = rc == KMPGPU_EINVAL && msg == std::string("kmpgpu_set_flowbits: ") + text && t.acting.empty() && t.tests.empty() && t.n_bits == 0;
    if (!ok) fprintf(stderr, "rc %d, message '%s' (wanted 'kmpgpu_set_flowbits: %s')\n", rc, msg.c_str(), text);
    return ok;
}

static bool packed(const Ops &ops, uint32_t n_bits, uint32_t n_rules, kmp_flowbit_tables *t)
{
    std::string msg;
    const int rc = kmp_pack_flowbits(ops.data(), (uint32_t)ops.size(), n_bits, n_rules, t, &msg);
    if (rc) fprintf(stderr, "rc %d, message '%s'\n", rc, msg.c_str());
    return rc == KMPGPU_OK;
}

static void refusals(void)
{
    const Ops one = {{0, 0, SET, 0}};
    CHECK(refused(one, 0, 1, "n_bits is 0, outside 1..32"));
    CHECK(refused(one, 33, 1, "n_bits is 33, outside 1..32"));
    {
        kmp_flowbit_tables t;
        std::string msg;
        CHECK(kmp_pack_flowbits(nullptr, 1, 1, 1, &t, &msg) == KMPGPU_EINVAL && msg == "kmpgpu_set_flowbits: ops is NULL");
    }
    CHECK(refused({{0, 0, SET, 0}, {2, 0, SET, 0}}, 1, 2, "op 1 names rule 2 of 2"));
    CHECK(refused({{0, 0, SET, 0}, {1, 3, ISSET, 0}}, 3, 2, "op 1 names bit 3 of 3"));
    CHECK(refused({{0, 0, 6, 0}}, 1, 1, "op 0: 6 is none of KMPGPU_FB_*"));
    CHECK(refused({{0, 0, SET, 7}}, 1, 1, "op 0: the reserved field is 7, not 0"));
    CHECK(refused({{0, 1, ISSET, 0}, {1, 1, ISNOTSET, 0}, {0, 1, ISNOTSET, 0}}, 2, 2, "op 2: rule 0 tests bit 1 both set and clear"));
    /* NOALERT does not look at its bit */
    kmp_flowbit_tables t;
    CHECK(packed({{0, 99, NOALERT, 0}}, 1, 1, &t) && t.tests == Words({0, 0, 1, 0}) && t.acting.empty());
    /* cycles of length 2 and 3, named from the lowest bit on them */
    CHECK(refused({{0, 0, ISSET, 0}, {0, 1, SET, 0}, {1, 1, ISNOTSET, 0}, {1, 0, UNSET, 0}}, 2, 2,
                  "the flow bits 0 -> 1 -> 0 form a cycle (a rule tests one and acts on the next)"));
    CHECK(refused({{0, 3, ISSET, 0}, {0, 1, SET, 0}, {1, 1, ISSET, 0}, {1, 2, SET, 0}, {2, 2, ISSET, 0}, {2, 3, TOGGLE, 0}, {2, 0, SET, 0}}, 4, 3,
                  "the flow bits 1 -> 2 -> 3 -> 1 form a cycle (a rule tests one and acts on the next)"));
    /* one rule that tests and acts on two bits crosswise is a cycle of length 2 */
    CHECK(refused({{0, 0, ISSET, 0}, {0, 1, ISSET, 0}, {0, 0, UNSET, 0}, {0, 1, UNSET, 0}}, 2, 1,
                  "the flow bits 0 -> 1 -> 0 form a cycle (a rule tests one and acts on the next)"));
}

static void tables(void)
{
    kmp_flowbit_tables t;
    /* a self-loop is no edge: fire once */
    CHECK(packed({{0, 0, ISNOTSET, 0}, {0, 0, SET, 0}}, 1, 1, &t));
    CHECK(t.n_bits == 1 && t.n_levels == 1 && t.level_of == Words({0}) && t.level_mask == Words({1}) && t.level_first == Words({0, 1}));
    CHECK(t.acting == Words({0, 0, 0, 2, 1, ID1, 0, 0}));          /* rule 0, no lower tests, self: tested clear, set: (1, 1) on bit 0 */
    CHECK(t.tests == Words({0, 1, 0, 0}));

    /* three levels, 0 -> 1 -> 2, with a bit nobody touches (3) and rules out of order in the op list */
    const Ops chain = {{2, 1, ISSET, 0}, {2, 2, SET, 0}, {0, 0, SET, 0}, {0, 0xFFFFFFFFu, NOALERT, 0}, {1, 0, ISSET, 0}, {1, 1, TOGGLE, 0}, {3, 2, ISNOTSET, 0},
                       {1, 1, ISNOTSET, 0}};
    CHECK(packed(chain, 4, 4, &t));
    CHECK(t.n_levels == 3 && t.level_of == Words({0, 1, 2, 0}) && t.level_mask == Words({9, 2, 4}) && t.level_first == Words({0, 1, 2, 3}));
    CHECK(t.acting == Words({0, 0, 0, 0, 1, ID1, 0, 0,                       /* level 0: rule 0 sets bit 0                                    */
                             1, 1, 0, 2, 2, ID1 & ~2u, 0, 0,                /* level 1: rule 1, bit 0 tested set below, own bit clear; toggle */
                             2, 2, 0, 0, 4, ID1, 0, 0}));                   /* level 2: rule 2, bit 1 tested set below; set bit 2             */
    CHECK(t.tests == Words({0, 0, 1, 0, 1, 2, 0, 0, 2, 0, 0, 0, 0, 4, 0, 0}));

    /* the longest path decides: 0 -> 2 directly and 0 -> 1 -> 2 */
    CHECK(packed({{0, 0, ISSET, 0}, {0, 2, SET, 0}, {0, 1, SET, 0}, {1, 1, ISSET, 0}, {1, 2, UNSET, 0}}, 3, 2, &t));
    CHECK(t.level_of == Words({0, 1, 2}) && t.level_first == Words({0, 0, 1, 3}));
    CHECK(t.acting == Words({0, 1, 0, 0, 2, ID1, 0, 0,                       /* level 1: rule 0 on bit 1 alone                                */
                             0, 1, 0, 0, 4, ID1, 0, 0,                       /* level 2: rule 0 sets bit 2, then                              */
                             1, 2, 0, 0, 0, ID1 & ~4u, 0, 0}));             /*          rule 1 unsets it                                     */

    /* a rule's actions compose in the order given: set then toggle is unset, toggle then set is set; two rules on one level in index order */
    CHECK(packed({{1, 0, TOGGLE, 0}, {1, 0, SET, 0}, {0, 0, SET, 0}, {0, 0, TOGGLE, 0}, {0, 1, UNSET, 0}}, 2, 2, &t));
    CHECK(t.n_levels == 1 && t.level_mask == Words({3}));
    CHECK(t.acting == Words({0, 0, 0, 0, 0, ID1 & ~3u, 0, 0,
                             1, 0, 0, 0, 1, ID1, 0, 0}));
    /* tests only: no record, and 32 bits are fine */
    CHECK(packed({{0, 31, ISSET, 0}}, 32, 1, &t) && t.acting.empty() && t.level_first == Words({0, 0}) && t.tests == Words({0x80000000u, 0, 0, 0}));
    (void)ID0;
}

/* ---- the file parser ---------------------------------------------------------------------------------------------------------------- */
static std::string g_dir;

static int parse_text(const char *text, uint32_t n_rules, kmp_flowbits *out, std::string *err)
{
    const std::string path = g_dir + "/flowbits.txt";
    FILE *fp = fopen(path.c_str(), "wb");
    if (!fp) { perror(path.c_str()); g_failed++; return -100; }
    fputs(text, fp);
    fclose(fp);
    char buf[KMP_FLOWBITS_ERRBUF];
    memset(buf, 'x', sizeof buf);
    const int rc = kmp_flowbits_parse(path.c_str(), n_rules, out, buf);
    *err = buf;
    return rc;
}

static bool parse_refused(const char *text, uint32_t n_rules, const char *want)
{
    kmp_flowbits f;
    std::string err;
    const int rc = parse_text(text, n_rules, &f, &err);
    const bool ok = rc == KMPHOST_EINVAL && err == want && f.ops == nullptr && f.n == 0;
    if (!ok) fprintf(stderr, "rc %d, message '%s' (wanted '%s')\n", rc, err.c_str(), want);
    kmp_flowbits_free(&f);
    return ok;
}

static void parser(void)
{
    kmp_flowbits f;
    std::string err;
    CHECK(parse_text("# login, then the command\n\n0 set:logged.in noalert\n  1 isset:logged.in\n2\tunset:logged.in   toggle:x-1 isnotset:A_b\n0 isnotset:x-1\n", 3, &f, &err) == KMPHOST_OK);
    CHECK(err.empty() && f.n == 7 && f.n_bits == 3);
    CHECK(!strcmp(f.names[0], "logged.in") && !strcmp(f.names[1], "x-1") && !strcmp(f.names[2], "A_b"));
    const kmp_flowbit_op want[7] = {{0, 0, KMP_FB_SET, 0}, {0, 0, KMP_FB_NOALERT, 0}, {1, 0, KMP_FB_ISSET, 0}, {2, 0, KMP_FB_UNSET, 0}, {2, 1, KMP_FB_TOGGLE, 0},
                                    {2, 2, KMP_FB_ISNOTSET, 0}, {0, 1, KMP_FB_ISNOTSET, 0}};
    CHECK(f.n == 7 && !memcmp(f.ops, want, sizeof want));
    /* what the parser gives is what the packer takes: A_b -> x-1 -> logged.in, and A_b -> logged.in */
    kmp_flowbit_tables t;
    std::string msg;
    CHECK(kmp_pack_flowbits((const kmpgpu_flowbit_op *)f.ops, f.n, f.n_bits, 3, &t, &msg) == KMPGPU_OK && t.level_of == Words({2, 1, 0}));
    kmp_flowbits_free(&f);
    CHECK(f.ops == nullptr && f.n == 0);
    /* noalert alone: one bit; an empty file: no ops */
    CHECK(parse_text("0 noalert\n", 1, &f, &err) == KMPHOST_OK && f.n == 1 && f.n_bits == 1);
    kmp_flowbits_free(&f);
    CHECK(parse_text("# nothing\n", 1, &f, &err) == KMPHOST_OK && f.n == 0 && f.ops == nullptr);
    kmp_flowbits_free(&f);
    /* a name of 31 characters, and 32 names */
    CHECK(parse_text("0 set:abcdefghijklmnopqrstuvwxyz01234\n", 1, &f, &err) == KMPHOST_OK && strlen(f.names[0]) == 31);
    kmp_flowbits_free(&f);
    std::string many = "0";
    for (int i = 0; i < 32; i++) many += " set:n" + std::to_string(i);
    CHECK(parse_text((many + "\n").c_str(), 1, &f, &err) == KMPHOST_OK && f.n_bits == 32 && !strcmp(f.names[31], "n31"));
    kmp_flowbits_free(&f);

    CHECK(parse_refused("0 set:a\n\nx set:a\n", 1, "line 3: 'x' is not a rule index"));
    CHECK(parse_refused("0 set:a\n-1 set:a\n", 1, "line 2: '-1' is not a rule index"));
    CHECK(parse_refused("# c\n1 set:a\n", 1, "line 2: rule 1 of 1"));
    CHECK(parse_refused("0 set:a\n0\n", 1, "line 2: rule 0 has no word"));
    CHECK(parse_refused("0 seta\n", 1, "line 1: 'seta' is none of set:<name> unset:<name> toggle:<name> isset:<name> isnotset:<name> noalert"));
    CHECK(parse_refused("0 clear:a\n", 1, "line 1: 'clear:a' is none of set:<name> unset:<name> toggle:<name> isset:<name> isnotset:<name> noalert"));
    CHECK(parse_refused("0 noalert:a\n", 1, "line 1: 'noalert:a' is none of set:<name> unset:<name> toggle:<name> isset:<name> isnotset:<name> noalert"));
    CHECK(parse_refused("0 set:\n", 1, "line 1: 'set:': a name is 1..31 characters of [A-Za-z0-9_.-]"));
    CHECK(parse_refused("0 set:a+b\n", 1, "line 1: 'set:a+b': a name is 1..31 characters of [A-Za-z0-9_.-]"));
    CHECK(parse_refused("0 set:abcdefghijklmnopqrstuvwxyz012345\n", 1, "line 1: 'set:abcdefghijklmnopqrstuvwxyz012345': a name is 1..31 characters of [A-Za-z0-9_.-]"));
    CHECK(parse_refused((many + "\n0 isset:n0\n0 set:one.more\n").c_str(), 1, "line 3: 'set:one.more' is name 33: at most 32 flow bits"));
    CHECK(parse_refused("0 isset:a\n1 isnotset:a\n0 set:b isnotset:a\n", 2, "line 3: rule 0 tests a both set and clear"));
    CHECK(parse_refused("0 isset:a set:b\n1 isset:b unset:a\n", 2, "the flow bits a -> b -> a form a cycle"));
    CHECK(parse_refused("0 isset:c set:a\n1 isset:a set:b\n2 isnotset:b toggle:c\n", 3, "the flow bits c -> a -> b -> c form a cycle"));
    {
        char buf[KMP_FLOWBITS_ERRBUF];
        CHECK(kmp_flowbits_parse((g_dir + "/no such file").c_str(), 1, &f, buf) == KMPHOST_EIO && f.ops == nullptr);
    }
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s <directory>\n", argv[0]); return 2; }
    g_dir = argv[1];
    refusals();
    tables();
    parser();
    if (g_failed) { fprintf(stderr, "%d checks failed\n", g_failed); return 1; }
    printf("flowbits driver ok\n");
    return 0;
}
