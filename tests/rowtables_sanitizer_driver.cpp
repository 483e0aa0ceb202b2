/* Built with -fsanitize=address,undefined by tests/test_rowtables_host.py: drives the packers of the rules, windows, relations and chains
 * tables (csrc/kmp_rowtables.cpp) without a device.  Every expected table below is written out by hand from the description of the
 * device form in csrc/kmp_launch.h, none is computed by the code under test. */
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "kmp_rowtables.h"

typedef std::vector<uint32_t> Words;

static int g_failed = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "CHECK failed: %s (line %d)\n", #c, __LINE__); g_failed++; } } while (0)

static const uint32_t N = KMPGPU_RULE_NOT;
static const uint32_t F = 0x80000000u;                        /* the fold bit of a record */
static const uint32_t MIN = 0x80000000u, MAX = 0x7FFFFFFFu;   /* INT32_MIN, INT32_MAX as the records hold them */

/* refused with KMPGPU_EINVAL and the whole message of that setter */
static bool refused(int rc, const std::string &msg, const char *setter, const char *text)
{
    const bool ok = rc == KMPGPU_EINVAL && msg == std::string(setter) + ": " + text;
    if (!ok) fprintf(stderr, "rc %d, message '%s' (wanted '%s: %s')\n", rc, msg.c_str(), setter, text);
    return ok;
}

/* ---- rules: 8 patterns + 1 relation + 1 chain = rows 0 .. 9 -------------------------------------------------------------------------- */
static const uint32_t NP = 8, NR = 1, NC = 1, ROWS = 10;

/* a rule as the comment in kmp_launch.h says the kernel reads it: the head's two terms, then the quads [head.x, head.y) */
static bool packed_rule_holds(const Words &heads, const Words &quads, uint32_t r, uint32_t hit)
{
    std::vector<uint32_t> terms = {heads[4 * r + 2], heads[4 * r + 3]};
    for (uint32_t q = heads[4 * r]; q < heads[4 * r + 1]; q++)
        for (int k = 0; k < 4; k++) terms.push_back(quads[4 * q + k]);
    for (const uint32_t t : terms)
        if ((((hit >> (t & ~N)) & 1u) != 0) == ((t & N) != 0)) return false;
    return true;
}

static bool direct_rule_holds(const Words &terms, uint32_t hit)
{
    for (const uint32_t t : terms) {
        const bool in = ((hit >> (t & 0x7FFFFFFFu)) & 1u) != 0;
        if (t & N ? in : !in) return false;
    }
    return true;
}

static void rules(void)
{
    const std::vector<Words> rule = {
        {3},                                /* 1 term: head only, the term twice                                   */
        {1, N | 2},                         /* 2 terms: head only                                                  */
        {4, 5, 6},                          /* 3 terms: one quad, padded with repeats of its first term            */
        {0, 1, 2, 3, 4, 5},                 /* 6 terms: exactly one full quad                                      */
        {0, 1, 2, 3, 4, 5, 6},              /* 7 terms: two quads                                                  */
        {N | 7, 2, N | 0, 9, 5},            /* negated and plain terms mixed in file order: the plain ones first   */
        {N | 4, N | 8},                     /* all negated                                                         */
    };
    const Words want_heads = {
        0, 0, 3, 3,
        0, 0, 1, N | 2,
        0, 1, 4, 5,
        1, 2, 0, 1,
        2, 4, 0, 1,
        4, 5, 2, 9,
        5, 5, N | 4, N | 8,
    };
    const Words want_quads = {
        6, 6, 6, 6,
        2, 3, 4, 5,
        2, 3, 4, 5,
        6, 6, 6, 6,
        5, N | 7, N | 0, 5,
    };
    Words off = {0}, terms;
    for (const Words &r : rule) { terms.insert(terms.end(), r.begin(), r.end()); off.push_back((uint32_t)terms.size()); }
    Words heads, quads;
    std::string msg;
    CHECK(kmp_pack_rules(off.data(), terms.data(), (uint32_t)rule.size(), NP, NR, NC, &heads, &quads, &msg) == KMPGPU_OK);
    CHECK(heads == want_heads);
    CHECK(quads == want_quads);
    /* the packed form decides what the AND / NOT of the original terms decides, over every assignment of hits to the rows */
    if (heads.size() == 4 * rule.size())
        for (uint32_t r = 0; r < rule.size(); r++)
            for (uint32_t hit = 0; hit < (1u << ROWS); hit++)
                if (packed_rule_holds(heads, quads, r, hit) != direct_rule_holds(rule[r], hit)) { CHECK(!"packed rule differs"); hit = 1u << ROWS; }

    /* a single rule of one or two terms has no quads at all */
    const Words off1 = {0, 1}, t1 = {ROWS - 1};                          /* (the last row is a valid term) */
    CHECK(kmp_pack_rules(off1.data(), t1.data(), 1, NP, NR, NC, &heads, &quads, &msg) == KMPGPU_OK);
    CHECK((heads == Words{0, 0, ROWS - 1, ROWS - 1}) && quads.empty());
    const Words t1n = {N | (ROWS - 1)};
    CHECK(kmp_pack_rules(off1.data(), t1n.data(), 1, NP, NR, NC, &heads, &quads, &msg) == KMPGPU_OK);
    CHECK((heads == Words{0, 0, N | (ROWS - 1), N | (ROWS - 1)}) && quads.empty());

    /* refused */
    const Words two = {0, 1};
    const Words off_bad0 = {1, 2};
    CHECK(refused(kmp_pack_rules(off_bad0.data(), two.data(), 1, NP, NR, NC, &heads, &quads, &msg), msg, "kmpgpu_set_rules", "rule_off[0] is 1, not 0"));
    const Words off_dec = {0, 2, 1};
    CHECK(refused(kmp_pack_rules(off_dec.data(), two.data(), 2, NP, NR, NC, &heads, &quads, &msg), msg, "kmpgpu_set_rules", "rule_off decreases at rule 1"));
    const Words off_empty = {0, 1, 1, 2};
    CHECK(refused(kmp_pack_rules(off_empty.data(), two.data(), 3, NP, NR, NC, &heads, &quads, &msg), msg, "kmpgpu_set_rules", "rule 1 has no terms"));
    const Words t_rows = {0, ROWS}, t_rows_not = {0, N | ROWS}, off2 = {0, 2};
    CHECK(refused(kmp_pack_rules(off2.data(), t_rows.data(), 1, NP, NR, NC, &heads, &quads, &msg), msg, "kmpgpu_set_rules",
                  "rule 0: term 1 names row 10 of 8 patterns + 1 relations + 1 chains"));
    CHECK(refused(kmp_pack_rules(off2.data(), t_rows_not.data(), 1, NP, NR, NC, &heads, &quads, &msg), msg, "kmpgpu_set_rules",
                  "rule 0: term 1 names row 10 of 8 patterns + 1 relations + 1 chains"));
    CHECK(refused(kmp_pack_rules(nullptr, two.data(), 1, NP, NR, NC, &heads, &quads, &msg), msg, "kmpgpu_set_rules", "NULL rule arrays"));
}

/* ---- relations and chains: 4 patterns, 1 and 3 of the nocase set ---------------------------------------------------------------------- */
static const uint8_t FOLD[4] = {0, 1, 0, 1};

static void relations(void)
{
    const kmpgpu_relation rel[] = {
        {0, 2, 0, 10},                      /* the fold bit on neither,          */
        {1, 2, -3, 3},                      /* on a,                             */
        {2, 3, INT32_MIN, INT32_MAX},       /* on b,                             */
        {3, 1, 5, 5},                       /* on both; dmin == dmax             */
    };
    const Words want = {
        0, 2, 0, 10,
        F | 1, 2, 0xFFFFFFFDu, 3,
        2, F | 3, MIN, MAX,
        F | 3, F | 1, 5, 5,
    };
    Words out;
    std::string msg;
    CHECK(kmp_pack_relations(rel, 4, 4, 0, FOLD, &out, &msg) == KMPGPU_OK);
    CHECK(out == want);

    const kmpgpu_relation above[] = {{0, 1, 6, 5}};
    CHECK(refused(kmp_pack_relations(above, 1, 4, 0, FOLD, &out, &msg), msg, "kmpgpu_set_relations", "relation 0: dmin 6 lies above dmax 5"));
    const kmpgpu_relation a_out[] = {{0, 1, 0, 0}, {4, 1, 0, 0}}, b_out[] = {{3, 4, 0, 0}};
    CHECK(refused(kmp_pack_relations(a_out, 2, 4, 0, FOLD, &out, &msg), msg, "kmpgpu_set_relations", "relation 1 names pattern 4 of 4"));
    CHECK(refused(kmp_pack_relations(b_out, 1, 4, 0, FOLD, &out, &msg), msg, "kmpgpu_set_relations", "relation 0 names pattern 4 of 4"));
    /* the 2^31 rows a rule term can name: decided on the counts, the one-element array is never read behind its end */
    CHECK(refused(kmp_pack_relations(rel, 0x7FFFFFFCu, 4, 0, FOLD, &out, &msg), msg, "kmpgpu_set_relations",
                  "4 patterns + 2147483644 relations do not fit the 2^31 rows a rule term can name"));
    CHECK(refused(kmp_pack_relations(rel, 0x7FFFFFFBu, 4, 1, FOLD, &out, &msg), msg, "kmpgpu_set_relations",
                  "4 patterns + 2147483643 relations + the chains do not fit the 2^31 rows a rule term can name"));
    CHECK(refused(kmp_pack_relations(nullptr, 1, 4, 0, FOLD, &out, &msg), msg, "kmpgpu_set_relations", "rel is NULL"));
}

static void chains(void)
{
    static_assert(KMPGPU_CHAIN_MAX == 8, "the tables below are written for 8 records per chain");
    const kmpgpu_chain_link links[] = {
        /* chain 0: 2 contents */
        {1, INT32_MIN, INT32_MAX}, {2, -4, 7},
        /* chain 1: KMPGPU_CHAIN_MAX contents */
        {0, INT32_MIN, INT32_MAX}, {1, 1, 11}, {2, 2, 12}, {3, 3, 13}, {0, 4, 14}, {1, 5, 15}, {2, 6, 16}, {3, INT32_MIN, 17},
    };
    const uint32_t off[] = {0, 2, 10};
    const Words want = {
        F | 1, MIN, MAX, 2,
        2, 0xFFFFFFFCu, 7, 2,   2, 0xFFFFFFFCu, 7, 2,   2, 0xFFFFFFFCu, 7, 2,   2, 0xFFFFFFFCu, 7, 2,
        2, 0xFFFFFFFCu, 7, 2,   2, 0xFFFFFFFCu, 7, 2,   2, 0xFFFFFFFCu, 7, 2,
        0, MIN, MAX, 8,
        F | 1, 1, 11, 8,   2, 2, 12, 8,   F | 3, 3, 13, 8,   0, 4, 14, 8,   F | 1, 5, 15, 8,   2, 6, 16, 8,   F | 3, MIN, 17, 8,
    };
    Words out;
    std::string msg;
    CHECK(kmp_pack_chains(off, links, 2, 4, 0, FOLD, &out, &msg) == KMPGPU_OK);
    CHECK(out == want);

    const uint32_t off_one[] = {0, 1}, off_nine[] = {0, 9}, off_two[] = {0, 2};
    const kmpgpu_chain_link nine[9] = {{0, INT32_MIN, INT32_MAX}, {1, 0, 1}, {1, 0, 1}, {1, 0, 1}, {1, 0, 1}, {1, 0, 1}, {1, 0, 1}, {1, 0, 1}, {1, 0, 1}};
    CHECK(refused(kmp_pack_chains(off_one, nine, 1, 4, 0, FOLD, &out, &msg), msg, "kmpgpu_set_chains", "chain 0 has 1 contents, not 2 .. 8"));
    CHECK(refused(kmp_pack_chains(off_nine, nine, 1, 4, 0, FOLD, &out, &msg), msg, "kmpgpu_set_chains", "chain 0 has 9 contents, not 2 .. 8"));
    const kmpgpu_chain_link lo_bound[] = {{0, 0, INT32_MAX}, {1, 0, 1}}, hi_bound[] = {{0, INT32_MIN, 5}, {1, 0, 1}};
    CHECK(refused(kmp_pack_chains(off_two, lo_bound, 1, 4, 0, FOLD, &out, &msg), msg, "kmpgpu_set_chains", "chain 0: its first content is relative to nothing and carries no bounds (a window places it)"));
    CHECK(refused(kmp_pack_chains(off_two, hi_bound, 1, 4, 0, FOLD, &out, &msg), msg, "kmpgpu_set_chains", "chain 0: its first content is relative to nothing and carries no bounds (a window places it)"));
    const uint32_t off_dec[] = {0, 2, 1}, off_bad0[] = {1, 3};
    CHECK(refused(kmp_pack_chains(off_dec, links, 2, 4, 0, FOLD, &out, &msg), msg, "kmpgpu_set_chains", "chain_off decreases at chain 1"));
    CHECK(refused(kmp_pack_chains(off_bad0, links, 1, 4, 0, FOLD, &out, &msg), msg, "kmpgpu_set_chains", "chain_off[0] is 1, not 0"));
    const kmpgpu_chain_link p_out[] = {{0, INT32_MIN, INT32_MAX}, {4, 0, 1}}, above[] = {{0, INT32_MIN, INT32_MAX}, {1, 2, 1}};
    CHECK(refused(kmp_pack_chains(off_two, p_out, 1, 4, 0, FOLD, &out, &msg), msg, "kmpgpu_set_chains", "chain 0 names pattern 4 of 4"));
    CHECK(refused(kmp_pack_chains(off_two, above, 1, 4, 0, FOLD, &out, &msg), msg, "kmpgpu_set_chains", "chain 0: dmin 2 lies above dmax 1"));
    CHECK(refused(kmp_pack_chains(off_two, links, 0x7FFFFFFAu, 4, 2, FOLD, &out, &msg), msg, "kmpgpu_set_chains",
                  "4 patterns + 2 relations + 2147483642 chains do not fit the 2^31 rows a rule term can name"));
    CHECK(refused(kmp_pack_chains(nullptr, links, 1, 4, 0, FOLD, &out, &msg), msg, "kmpgpu_set_chains", "NULL chain arrays"));
}

static void windows(void)
{
    Words out = {1, 2, 3};
    std::string msg;
    const uint32_t first_d[] = {0, 0, 0}, last_d[] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    CHECK(kmp_pack_windows(first_d, last_d, 3, 3, &out, &msg) == KMPGPU_OK);
    CHECK(out.empty());                                                   /* every window the default: no table */
    const uint32_t first_1[] = {0, 0, 0}, last_1[] = {0xFFFFFFFFu, 0xFFFFFFFEu, 0xFFFFFFFFu};
    CHECK(kmp_pack_windows(first_1, last_1, 3, 3, &out, &msg) == KMPGPU_OK);
    CHECK((out == Words{0, 0xFFFFFFFFu, 0, 0xFFFFFFFEu, 0, 0xFFFFFFFFu}));  /* one that is not: the whole table */
    const uint32_t first_2[] = {7, 0, 4}, last_2[] = {7, 0xFFFFFFFFu, 90};
    CHECK(kmp_pack_windows(first_2, last_2, 3, 3, &out, &msg) == KMPGPU_OK);
    CHECK((out == Words{7, 7, 0, 0xFFFFFFFFu, 4, 90}));
    const uint32_t first_b[] = {0, 9, 0}, last_b[] = {1, 8, 1};
    CHECK(refused(kmp_pack_windows(first_b, last_b, 3, 3, &out, &msg), msg, "kmpgpu_set_windows", "pattern 1: first 9 lies behind last 8"));
    CHECK(refused(kmp_pack_windows(first_d, last_d, 2, 3, &out, &msg), msg, "kmpgpu_set_windows", "2 windows for 3 patterns"));
    CHECK(refused(kmp_pack_windows(first_d, nullptr, 3, 3, &out, &msg), msg, "kmpgpu_set_windows", "NULL window arrays"));
}

int main(void)
{
    rules();
    relations();
    chains();
    windows();
    if (g_failed) return 1;
    printf("rowtables driver ok\n");
    return 0;
}
