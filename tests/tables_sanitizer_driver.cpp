/* Built with -fsanitize=address,undefined by tests/test_host.py: drives the builder of the fused pass's tables
 * (csrc/kmp_tables.cpp) over the smallest pattern sets that reach each of its branches, and checks the STRUCTURE of
 * what it returns (who is counted where, sizes, orders) -- not a model of the kernel that reads the tables. */
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <set>
#include <string>
#include <vector>

#include "kmp_tables.h"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s: CHECK failed: %s (line %d)\n", set_name, #c, __LINE__); return false; } } while (0)

struct PatternSet {
    const char *name;
    std::vector<std::string> pats;          /* the whole list, file order */
    std::vector<uint32_t> members;          /* the ones of this set (kmpgpu_set_patterns splits a list in two sets) */
    /* what the set is there to reach; -1: not asked */
    int groups = -1, plain = -1, classed_min = -1, n_ones = -1, rest_long = -1, rest_short = -1;
    uint32_t bmask = 0;
    int in_rest = -1;                       /* this pattern index is on the rest list */
};

/* distinct strings of `len` lower-case letters behind `prefix` */
static std::string word(const std::string &prefix, uint32_t k, uint32_t len)
{
    std::string s = prefix;
    for (uint32_t b = 0; b < len; b++) { s.push_back((char)('a' + k % 26u)); k /= 26u; }
    return s;
}

static uint32_t bucket_class(const std::string &p)
{
    const uint32_t w24 = (uint8_t)p[0] | ((uint32_t)(uint8_t)p[1] << 8) | ((uint32_t)(uint8_t)p[2] << 16);
    return KMP_MULTI_HASH(w24 & KMP_MULTI_KEYMASK) >> KMP_MULTI_CLS_SHIFT;
}

static PatternSet all_of(const char *name, std::vector<std::string> pats)
{
    PatternSet s;
    s.name = name;
    s.pats = std::move(pats);
    for (uint32_t i = 0; i < s.pats.size(); i++) s.members.push_back(i);
    return s;
}

static std::vector<PatternSet> make_sets()
{
    std::vector<PatternSet> sets;
    {   /* members are indices into the list, not positions in the set */
        PatternSet s = all_of("two distinct patterns", {"abcd", "Q", "abcdefghij"});
        s.members = {0, 2};
        s.groups = 1; s.plain = 1; s.n_ones = 0; s.bmask = KMP_MULTI_KEYMASK; s.rest_long = 0; s.rest_short = 0;
        sets.push_back(s);
    }
    {
        PatternSet s = all_of("one eligible pattern plus 1-byte patterns", {"a", "needle", "b", "a"});
        s.groups = 0;
        sets.push_back(s);
    }
    {
        PatternSet s = all_of("duplicates of one pattern", {"same", "same", "same"});
        s.groups = 0;
        sets.push_back(s);
    }
    {
        std::vector<std::string> p;
        for (uint32_t k = 0; k < 9; k++) p.push_back(word("", k, 2));
        PatternSet s = all_of("nine 2-byte patterns", p);
        s.groups = 1; s.plain = 1; s.bmask = 0xFFFFu;
        sets.push_back(s);
    }
    {
        PatternSet s = all_of("five 1-byte patterns, two eligible ones", {"a", "b", "host", "c", "d", "e", "get", "b"});
        s.groups = 1; s.plain = 1; s.n_ones = 4; s.rest_long = 0; s.rest_short = 1; s.in_rest = 5; s.bmask = KMP_MULTI_KEYMASK;
        sets.push_back(s);
    }
    {
        std::vector<std::string> p;
        for (uint32_t k = 0; k < 257; k++) p.push_back(word("", k, 4));
        PatternSet s = all_of("257 distinct 4-byte patterns", p);
        s.plain = 0; s.classed_min = 1;
        sets.push_back(s);
    }
    {
        std::vector<std::string> p;
        for (uint32_t k = 0; k < 257; k++) p.push_back(word("", k, 4));
        p.push_back("x");
        PatternSet s = all_of("257 distinct patterns, no 2-byte one, a 1-byte pattern", p);
        s.plain = 1; s.classed_min = 1; s.n_ones = 1;
        sets.push_back(s);
    }
    {   /* one bucket is one class: a class holds 256 patterns, so the second group opens there */
        std::vector<std::string> p;
        for (uint32_t k = 0; k < 600; k++) p.push_back(word("abc", k, 2));
        PatternSet s = all_of("600 patterns that share their first three bytes", p);
        s.plain = 0; s.classed_min = 2;
        sets.push_back(s);
    }
    {   /* three buckets of three classes, 200 patterns each: no class is full, the entry list (KMP_MULTI_MAX_ENTRIES) is */
        std::vector<std::string> heads;
        std::set<uint32_t> seen;
        for (char b1 = 'a'; b1 <= 'z' && heads.size() < 3; b1++)
            for (char b2 = 'a'; b2 <= 'z' && heads.size() < 3; b2++) {
                const std::string h{'a', b1, b2};
                if (seen.insert(bucket_class(h)).second) heads.push_back(h);
            }
        std::vector<std::string> p;
        for (uint32_t k = 0; k < 600 && heads.size() == 3; k++) p.push_back(word(heads[k % 3], k / 3, 2));
        PatternSet s = all_of("600 patterns in three buckets of three classes", p);
        s.plain = 0; s.classed_min = 2;
        sets.push_back(s);
    }
    {
        std::vector<std::string> p;
        for (uint32_t k = 0; k < 65537; k++) p.push_back(k & 1 ? "abcd" : "xy");
        p.push_back("ninebytes");
        PatternSet s = all_of("65 538 patterns whose last is a new 9-byte pattern", p);
        s.groups = 1; s.rest_long = 1; s.rest_short = 0; s.in_rest = 65537;
        sets.push_back(s);
    }
    return sets;
}

static std::vector<kmp_pattern_dev> device_patterns(const PatternSet &ps)
{
    std::vector<kmp_pattern_dev> host(ps.pats.size());
    for (size_t i = 0; i < ps.pats.size(); i++) {
        memset(&host[i], 0, sizeof host[i]);
        memcpy(host[i].pat, ps.pats[i].data(), ps.pats[i].size());
        host[i].m = (uint32_t)ps.pats[i].size();
    }
    return host;
}

static bool check_set(const PatternSet &ps)
{
    const char *set_name = ps.name;
    CHECK(!ps.pats.empty());
    const std::vector<kmp_pattern_dev> host = device_patterns(ps);
    kmp_set_tables t;
    CHECK(kmp_build_tables(host.data(), ps.members, &t));
    const size_t n = ps.members.size();

    /* the streaming passes' order: every member once, long patterns first */
    CHECK(t.ids.size() == n && (size_t)t.n_long + t.n_short == n);
    for (size_t k = 0; k < n; k++) CHECK((host[t.ids[k]].m >= 4) == (k < t.n_long));
    { std::vector<uint32_t> a(t.ids), b(ps.members); std::sort(a.begin(), a.end()); std::sort(b.begin(), b.end()); CHECK(a == b); }

    std::vector<uint32_t> counted(ps.pats.size(), 0u);
    uint32_t plain = 0, classed = 0, multi_unique = 0;
    for (size_t gi = 0; gi < t.groups.size(); gi++) {
        const kmp_group_tables &g = t.groups[gi];
        CHECK(g.ids.size() == g.rows.size() && g.uid_ids.size() == g.ids.size());
        CHECK(gi == 0 || g.n_ones == 0);                              /* 1-byte patterns ride along with the first group only */
        CHECK(g.n_ones <= KMP_MULTI_MAX_ONES && g.n_ones <= g.n_unique);
        CHECK(g.bmask == KMP_MULTI_KEYMASK || g.bmask == 0xFFFFu);
        std::set<std::string> uniq, uniq_long, ones;
        for (size_t k = 0; k < g.ids.size(); k++) {
            CHECK(g.ids[k] < ps.pats.size());
            counted[g.ids[k]]++;
            CHECK(g.rows[k] < g.n_unique);
            const std::string &p = ps.pats[g.ids[k]];
            if (p.size() == 1) { ones.insert(p); CHECK(g.rows[k] >= g.n_unique - g.n_ones); continue; }
            CHECK(g.rows[k] < g.n_unique - g.n_ones);
            uniq.insert(p);
            if (p.size() > KMP_MULTI_SHORT_LEN) uniq_long.insert(p);
        }
        CHECK(ones.size() == g.n_ones && uniq.size() == g.n_unique - g.n_ones);
        multi_unique += (uint32_t)uniq.size();
        /* row -> ids */
        CHECK(g.uid_first.size() == (size_t)g.n_unique + 1 && g.uid_first.front() == 0 && g.uid_first.back() == g.ids.size());
        for (uint32_t r = 0; r < g.n_unique; r++) CHECK(g.uid_first[r] <= g.uid_first[r + 1]);
        { std::vector<uint32_t> a(g.ids), b(g.uid_ids); std::sort(a.begin(), a.end()); std::sort(b.begin(), b.end()); CHECK(a == b); }
        /* sizes: kmp_device.h */
        if (g.classed) {
            classed++;
            CHECK(g.n_ones == 0 && g.n_unique <= 4u * KMP_MULTI_MAX_UNIQUE && g.cshift == KMP_MULTI_CLS_SHIFT);
            CHECK(g.tables.size() == KMP_MULTI_REC_W0 + KMP_MULTI_CLS_WORDS + uniq_long.size() * KMP_MULTI_CREC_WORDS);
        } else {
            plain++;
            CHECK(classed == 0);                                      /* plain groups come first */
            CHECK(g.n_unique - g.n_ones <= KMP_MULTI_MAX_UNIQUE);
            CHECK(g.cshift == uniq.size() - uniq_long.size());        /* its short patterns */
            CHECK(g.tables.size() == KMP_MULTI_REC_W0 + uniq_long.size() * KMP_MULTI_REC_WORDS);
        }
    }
    CHECK(t.n_multi_unique == multi_unique);

    if (t.groups.empty()) {
        /* nothing fused: no rest lists either, every pattern keeps the pass `ids` gives it */
        CHECK(t.rest.empty() && t.rest_long == 0 && t.rest_short == 0 && t.n_multi_unique == 0);
    } else {
        CHECK(t.n_multi_unique >= 2);
        CHECK(t.rest.size() == (size_t)t.rest_long + t.rest_short);
        for (size_t k = 0; k < t.rest.size(); k++) {
            CHECK(t.rest[k] < ps.pats.size());
            CHECK((host[t.rest[k]].m >= 4) == (k < t.rest_long));
            counted[t.rest[k]]++;
        }
        /* each member is counted by exactly one group or is on the rest list once; nobody else is */
        std::vector<uint32_t> want(ps.pats.size(), 0u);
        for (const uint32_t i : ps.members) want[i] = 1;
        CHECK(counted == want);
    }

    if (ps.groups >= 0) CHECK(t.groups.size() == (size_t)ps.groups);
    if (ps.plain >= 0) CHECK(plain == (uint32_t)ps.plain);
    if (ps.classed_min >= 0) CHECK(classed >= (uint32_t)ps.classed_min);
    if (ps.n_ones >= 0) CHECK(!t.groups.empty() && t.groups[0].n_ones == (uint32_t)ps.n_ones);
    if (ps.bmask) CHECK(!t.groups.empty() && t.groups[0].bmask == ps.bmask);
    if (ps.rest_long >= 0) CHECK(t.rest_long == (uint32_t)ps.rest_long);
    if (ps.rest_short >= 0) CHECK(t.rest_short == (uint32_t)ps.rest_short);
    if (ps.in_rest >= 0) CHECK(std::count(t.rest.begin(), t.rest.end(), (uint32_t)ps.in_rest) == 1);
    return true;
}

int main(void)
{
    const std::vector<PatternSet> sets = make_sets();
    for (const PatternSet &ps : sets)
        if (!check_set(ps)) return 1;
    printf("tables driver ok: %zu sets\n", sets.size());
    return 0;
}
