/* Built with -fsanitize=address,undefined by tests/test_links_host.py: drives the kmp_pack_rules entry that knows the links' rows
 * (csrc/kmp_rowtables.cpp) without a device.  Every expected table below is written out by hand from the description of the device form
 * in csrc/kmp_launch.h, none is computed by the code under test. */
#include <stdio.h>

#include <string>
#include <vector>

#include "kmp_rowtables.h"

typedef std::vector<uint32_t> Words;

static int g_failed = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "CHECK failed: %s (line %d)\n", #c, __LINE__); g_failed++; } } while (0)

static const uint32_t N = KMPGPU_RULE_NOT;

/* 2 patterns + 1 relation + 1 chain + 1 header predicate + 1 byte test + 1 expression = rows 0 .. 6, then 3 links = rows 7 .. 9 */
static const uint32_t NP = 2, NR = 1, NC = 1, NH = 1, NB = 1, NX = 1, NL = 3, L0 = 7;

static int pack(const std::vector<Words> &rule, uint32_t n_links, Words *heads, Words *quads, std::string *msg)
{
    Words off = {0}, terms;
    for (const Words &r : rule) {
        terms.insert(terms.end(), r.begin(), r.end());
        off.push_back((uint32_t)terms.size());
    }
    if (terms.empty()) terms.push_back(0);
    return kmp_pack_rules(off.data(), terms.data(), (uint32_t)rule.size(), NP, NR, NC, NH, NB, NX, n_links, heads, quads, msg);
}

static void tables(void)
{
    Words heads, quads;
    std::string msg;
    /* a link alone; a link negated beside a pattern; the three-buffer rule: two links and a header predicate, one link negated */
    CHECK(pack({{L0 + 2}, {N | L0, 1}, {L0, L0 + 1, 4, N | (L0 + 2)}}, NL, &heads, &quads, &msg) == KMPGPU_OK);
    CHECK((heads == Words{0, 0, L0 + 2, L0 + 2,                 /* one term: twice in the head, no quad                           */
                          0, 0, 1, N | L0,                      /* the plain term in front of the negated one                     */
                          0, 1, L0, L0 + 1}));                  /* two further terms: one quad                                    */
    CHECK((quads == Words{4, N | (L0 + 2), 4, 4}));             /* ... filled up with repeats of its first term                   */
    /* the last link is the last row; the row behind it is refused, and the message counts the links */
    CHECK(pack({{L0 + NL - 1}}, NL, &heads, &quads, &msg) == KMPGPU_OK);
    CHECK(pack({{0}, {1, L0 + NL}}, NL, &heads, &quads, &msg) == KMPGPU_EINVAL);
    CHECK(msg == "kmpgpu_set_rules: rule 1: term 1 names row 10 of 2 patterns + 1 relations + 1 chains + 1 header predicates + 1 byte tests + 1 expressions + 3 links");
    CHECK(pack({{N | (L0 + NL)}}, NL, &heads, &quads, &msg) == KMPGPU_EINVAL);
    /* without links the term is no row at all, and the message is the one of the entry without them */
    CHECK(pack({{L0}}, 0, &heads, &quads, &msg) == KMPGPU_EINVAL);
    CHECK(msg == "kmpgpu_set_rules: rule 0: term 0 names row 7 of 2 patterns + 1 relations + 1 chains + 1 header predicates + 1 byte tests + 1 expressions");
    Words h2, q2;
    std::string m2;
    const uint32_t off[] = {0, 2}, terms[] = {6, N | 0};
    CHECK(kmp_pack_rules(off, terms, 1, NP, NR, NC, NH, NB, NX, 0u, &heads, &quads, &msg) == KMPGPU_OK);
    CHECK(kmp_pack_rules(off, terms, 1, NP, NR, NC, NH, NB, NX, &h2, &q2, &m2) == KMPGPU_OK);
    CHECK(heads == h2 && quads == q2 && (heads == Words{0, 0, 6, N | 0}));
    /* the checks in front of the terms */
    CHECK(kmp_pack_rules(nullptr, terms, 1, NP, NR, NC, NH, NB, NX, NL, &heads, &quads, &msg) == KMPGPU_EINVAL);
    const uint32_t empty_rule[] = {0, 0};
    CHECK(kmp_pack_rules(empty_rule, terms, 1, NP, NR, NC, NH, NB, NX, NL, &heads, &quads, &msg) == KMPGPU_EINVAL);
    CHECK(msg == "kmpgpu_set_rules: rule 0 has no terms");
}

/* many rules of many link terms: the quads grow past one allocation, every index stays inside */
static void many(void)
{
    std::vector<Words> rule;
    for (uint32_t r = 0; r < 300; r++) {
        Words t;
        for (uint32_t j = 0; j <= r % 11; j++) t.push_back((j % 2 ? N : 0u) | (L0 + (r + j) % NL));
        rule.push_back(t);
    }
    Words heads, quads;
    std::string msg;
    CHECK(pack(rule, NL, &heads, &quads, &msg) == KMPGPU_OK);
    CHECK(heads.size() == 4 * rule.size() && quads.size() % 4 == 0);
    for (uint32_t r = 0; r < rule.size(); r++) {
        CHECK(heads[4 * r] <= heads[4 * r + 1] && heads[4 * r + 1] <= quads.size() / 4);
        /* the same set of terms, plain ones first */
        std::vector<uint32_t> got = {heads[4 * r + 2], heads[4 * r + 3]};
        for (uint32_t q = heads[4 * r]; q < heads[4 * r + 1]; q++)
            for (int k = 0; k < 4; k++) got.push_back(quads[4 * q + k]);
        for (const uint32_t t : got) {
            bool in = false;
            for (const uint32_t u : rule[r]) in = in || u == t;
            CHECK(in);
            CHECK((t & ~N) >= L0 && (t & ~N) < L0 + NL);
        }
        for (const uint32_t u : rule[r]) {
            bool in = false;
            for (const uint32_t t : got) in = in || u == t;
            CHECK(in);
        }
    }
}

int main(void)
{
    tables();
    many();
    if (g_failed) { fprintf(stderr, "%d checks failed\n", g_failed); return 1; }
    printf("links driver ok\n");
    return 0;
}
