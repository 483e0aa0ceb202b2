/* Built with -fsanitize=address,undefined by tests/test_regex_groups_host.py: drives the compiler and the interpreter of the expressions under
 * KMPGPU_RX_GROUPS (csrc/kmp_regex.cpp: kmp_regex_compile_groups, kmp_regex_search_groups), kmp_pack_regex_groups and the placeholder of
 * kmp_pack_regexes, without a device.
 *   argv[1]: the verdicts file in the format of tests/regex_sanitizer_driver.cpp (S texts, X <flags> <hex expression>, V <whole> <verdicts>).
 * An expression the linear compiler takes too must get the linear interpreter's verdict on every text. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "kmp_regex.h"
#include "kmp_rowtables.h"

typedef std::vector<uint32_t> Words;
typedef std::vector<uint8_t> Bytes;

static int g_failed = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "CHECK failed: %s (line %d)\n", #c, __LINE__); g_failed++; } } while (0)

static bool refused(int rc, const std::string &msg, const char *text)
{
    const bool ok = rc == KMPGPU_EINVAL && msg == text;
    if (!ok) fprintf(stderr, "rc %d, message '%s' (wanted '%s')\n", rc, msg.c_str(), text);
    return ok;
}

static Bytes unhex(const char *s)
{
    Bytes out;
    if (!strcmp(s, "-")) return out;
    for (; s[0] && s[1]; s += 2) {
        unsigned v = 0;
        sscanf(s, "%2x", &v);
        out.push_back((uint8_t)v);
    }
    return out;
}

static int compile(const char *expr, size_t len, uint32_t flags, kmp_regex_groups_table *t, std::string *msg)
{
    Bytes e(expr, expr + len);                              /* an exact-size heap copy: a read behind the expression is a finding */
    return kmp_regex_compile_groups(e.data(), e.size(), flags, t, msg);
}

static void verdicts(const char *path)
{
    FILE *f = fopen(path, "r");
    CHECK(f != nullptr);
    if (!f) return;
    std::vector<Bytes> texts;
    std::vector<char> line(1 << 20);
    kmp_regex_groups_table t;
    kmp_regex_table lin;
    std::string msg;
    bool have = false, have_lin = false;
    unsigned n_expr = 0, n_lin = 0;
    unsigned long long n_verdicts = 0, wrong = 0;
    while (fgets(line.data(), (int)line.size(), f)) {
        char *nl = strchr(line.data(), '\n');
        if (nl) *nl = 0;
        if (line[0] == 'S') texts.push_back(unhex(line.data() + 2));
        else if (line[0] == 'X') {
            unsigned flags = 0;
            int at = 0;
            sscanf(line.data() + 2, "%u %n", &flags, &at);
            const Bytes e = unhex(line.data() + 2 + at);
            have = compile((const char *)e.data(), e.size(), flags | KMPGPU_RX_GROUPS, &t, &msg) == KMPGPU_OK;
            if (!have) fprintf(stderr, "expression %u (%s) refused: %s\n", n_expr, line.data(), msg.c_str());
            CHECK(have);
            have_lin = kmp_regex_compile(e.data(), e.size(), flags, &lin, &msg) == KMPGPU_OK;
            if (have_lin) {
                n_lin++;
                CHECK(t.n == lin.n && t.n_rules == 0);
            }
            n_expr++;
        } else if (line[0] == 'V' && have) {
            const int whole = line[2] == '1';
            const char *v = line.data() + 4;
            CHECK(strlen(v) == texts.size());
            for (size_t i = 0; i < texts.size() && v[i]; i++) {
                size_t E = texts[i].size();
                if (!whole)
                    for (size_t z = 0; z < texts[i].size(); z++)
                        if (texts[i][z] == 0) { E = z; break; }
                Bytes exact(texts[i].begin(), texts[i].begin() + E);      /* nothing at or behind E is the interpreter's to read */
                const bool got = kmp_regex_search_groups(t, exact.data(), E);
                n_verdicts++;
                if (got != (v[i] == '1') && wrong++ < 10)
                    fprintf(stderr, "expression %u, text %zu, whole %d: got %d, the model says %c\n", n_expr - 1, i, whole, (int)got, v[i]);
                if (have_lin && got != kmp_regex_search(lin, exact.data(), E) && wrong++ < 10)
                    fprintf(stderr, "expression %u, text %zu, whole %d: the linear interpreter says otherwise\n", n_expr - 1, i, whole);
            }
        }
    }
    fclose(f);
    CHECK(wrong == 0);
    printf("%u expressions, %u of them linear too, %zu texts, %llu verdicts\n", n_expr, n_lin, texts.size(), n_verdicts);
}

static void refusals(void)
{
    static const struct { const char *expr; const char *msg; } bad[] = {
        {"(a|)", "position 3: an empty alternative"},
        {"()", "position 0: an empty group"},
        {"a(?:)", "position 1: an empty group"},
        {"a||b", "position 2: an empty alternative"},
        {"|a", "position 0: an empty alternative"},
        {"a|", "position 2: an empty alternative"},
        {"^a|b", "position 2: a top-level '|' beside ^ or $ (write ^(a|b)$: the anchors hold for the whole expression)"},
        {"a|b$", "position 1: a top-level '|' beside ^ or $ (write ^(a|b)$: the anchors hold for the whole expression)"},
        {"(?=a)", "position 0: '(?' opens no group but (?: ... ): look-around, names and inline flags are not part of the dialect"},
        {"a(?!b)", "position 1: '(?' opens no group but (?: ... ): look-around, names and inline flags are not part of the dialect"},
        {"(?<n>a)", "position 0: '(?' opens no group but (?: ... ): look-around, names and inline flags are not part of the dialect"},
        {"(?P<n>a)", "position 0: '(?' opens no group but (?: ... ): look-around, names and inline flags are not part of the dialect"},
        {"(?i)a", "position 0: '(?' opens no group but (?: ... ): look-around, names and inline flags are not part of the dialect"},
        {"(?", "position 0: '(?' opens no group but (?: ... ): look-around, names and inline flags are not part of the dialect"},
        {"(a", "position 0: unterminated group"},
        {"a(b|c", "position 1: unterminated group"},
        {"(", "position 0: unterminated group"},
        {"a)", "position 1: ')' without its opening (write \\))"},
        {"(a$)", "position 2: '$' anywhere but last"},
        {"(^a)", "position 1: '^' anywhere but first"},
        {"(*a)", "position 1: a quantifier on nothing"},
        {"a|+", "position 2: a quantifier on nothing"},
        {"(a)**", "position 4: a quantifier on a quantifier"},
        {"(a)+?", "position 4: a quantifier on a quantifier"},
        {"a**", "position 2: a quantifier on a quantifier"},
        {"(a){0}", "position 3: {n,m} needs m >= 1"},
        {"(a{8}){8}", "position 0: more than 63 positions"},
        {"(a|b){32}", "position 0: more than 63 positions"},
        {"a{63}(b)", "position 5: more than 63 positions"},
        {"(a{32}|b{31}c)", "position 12: more than 63 positions"},
        {"a{64}", "position 0: more than 63 positions"},
        {"(ab|cd){2,5}e", "position 0: needs 9 edge rules, more than 8"},
        {"((((((((((((((((((((((((((((((((((a))))))))))))))))))))))))))))))))))", "position 32: groups nested deeper than 32"},
        {"", "position 0: zero elements"},
        {"^$", "position 1: zero elements"},
    };
    kmp_regex_groups_table t;
    kmp_regex_table lin;
    std::string msg;
    for (const auto &b : bad)
        if (!refused(compile(b.expr, strlen(b.expr), 0, &t, &msg), msg, b.msg)) { fprintf(stderr, "  (expression '%s')\n", b.expr); g_failed++; }
    /* without the flag ( ) | are what they were */
    CHECK(refused(kmp_regex_compile((const uint8_t *)"a(b", 3, 0, &lin, &msg), msg, "position 1: '(' is reserved: groups and alternation are not part of the dialect"));
    CHECK(refused(kmp_regex_compile((const uint8_t *)"ab)", 3, 0, &lin, &msg), msg, "position 2: ')' is reserved: groups and alternation are not part of the dialect"));
    CHECK(refused(kmp_regex_compile((const uint8_t *)"a|b", 3, 0, &lin, &msg), msg, "position 1: '|' is reserved: groups and alternation are not part of the dialect"));
}

static void tables(void)
{
    static const struct { const char *expr; uint32_t n, rules; } want[] = {
        {"(GET|POST|HEAD|PUT) /", 16, 1}, {"(\\.\\./){3,}", 9, 1}, {"(cmd|powershell)(\\.exe)? ", 18, 2}, {"(ab|cd){2,4}e", 17, 7},
        {".{0,60}(a|b)7", 63, 1}, {"([ab].|7.){2,4}[^=]([aA]|.=)", 20, 8}, {"(ab|cd){2,4}e(f|gh)", 20, 8}, {"(?:ab){2}", 4, 0}, {"ab{0,2}\\d+c*d{2,}", 7, 0},
    };
    kmp_regex_groups_table t;
    std::string msg;
    for (const auto &w : want) {
        CHECK(compile(w.expr, strlen(w.expr), 0, &t, &msg) == KMPGPU_OK);
        if (t.n != w.n || t.n_rules != w.rules) { fprintf(stderr, "'%s': %u positions, %u rules\n", w.expr, t.n, t.n_rules); g_failed++; }
    }
    /* (GET|POST|HEAD|PUT) /: the last byte of the first three words jumps to the blank; PUT's shifts onto it */
    CHECK(compile("(GET|POST|HEAD|PUT) /", 21, 0, &t, &msg) == KMPGPU_OK);
    CHECK(t.src[0] == (1ull << 2 | 1ull << 6 | 1ull << 10) && t.dst[0] == 1ull << 14 && t.first == (1ull | 1ull << 3 | 1ull << 7 | 1ull << 11));
    CHECK(t.opt == 0 && t.rep == 0 && !t.bol && !t.eol && (t.shift & (1ull << 2)) == 0 && (t.shift & (1ull << 13)) != 0);
    /* the linear tables of the same expression: opt and rep are the same sets */
    kmp_regex_table lin;
    CHECK(compile("^ab{0,2}\\d+c*d{2,}$", 19, 0, &t, &msg) == KMPGPU_OK && kmp_regex_compile((const uint8_t *)"^ab{0,2}\\d+c*d{2,}$", 19, 0, &lin, &msg) == KMPGPU_OK);
    CHECK(t.opt == lin.opt && t.rep == lin.rep && t.bol && t.eol && t.n == lin.n && t.B['d'] == lin.B['d']);
}

static void packers(void)
{
    /* 2 KMP_RX_TILE + 1 expressions, flagged and unflagged taking turns */
    const uint32_t N = 2u * KMP_RX_TILE + 1u;
    const char *flagged = "(GET|POST|HEAD|PUT) /", *unflagged = "ab+$", *dummy = "x";
    std::vector<const uint8_t *> mixed(N), alone(N);
    Words len(N), len_alone(N), flags(N), flags_alone(N, 0u), gate(N, 0u);
    for (uint32_t q = 0; q < N; q++) {
        const bool fl = q % 2u == 0u;
        mixed[q] = (const uint8_t *)(fl ? flagged : unflagged); len[q] = (uint32_t)strlen((const char *)mixed[q]);
        alone[q] = (const uint8_t *)(fl ? dummy : unflagged); len_alone[q] = (uint32_t)strlen((const char *)alone[q]);
        flags[q] = fl ? KMPGPU_RX_GROUPS | (q % 4u == 0u ? KMPGPU_RX_GATED : 0u) : 0u;
        gate[q] = (flags[q] & KMPGPU_RX_GATED) ? 2u : 0u;
    }
    Words got, ref, grp;
    std::string msg;
    uint32_t ng = 0;
    CHECK(kmp_pack_regexes(mixed.data(), len.data(), flags.data(), gate.data(), N, 3, 1, 1, 1, 1, &got, &msg) == KMPGPU_OK);
    CHECK(kmp_pack_regexes(alone.data(), len_alone.data(), flags_alone.data(), nullptr, N, 3, 1, 1, 1, 1, &ref, &msg) == KMPGPU_OK);
    CHECK(got.size() == 3u * KMP_RX_TILE_WORDS && ref.size() == got.size());
    if (got.size() == ref.size() && got.size() == 3u * KMP_RX_TILE_WORDS)
        for (uint32_t q = 0; q < N; q++) {
            const uint32_t *tg = got.data() + (size_t)(q / KMP_RX_TILE) * KMP_RX_TILE_WORDS, *tr = ref.data() + (size_t)(q / KMP_RX_TILE) * KMP_RX_TILE_WORDS;
            const uint32_t qi = q % KMP_RX_TILE;
            const uint32_t *rec = tg + 512u * KMP_RX_TILE + 8u * qi, *rref = tr + 512u * KMP_RX_TILE + 8u * qi;
            bool same = memcmp(rec, rref, 32) == 0, zero = true;
            for (uint32_t c = 0; c < 256u; c++) {
                const uint32_t w = 2u * (c * KMP_RX_TILE + qi);
                same = same && tg[w] == tr[w] && tg[w + 1] == tr[w + 1];
                zero = zero && tg[w] == 0 && tg[w + 1] == 0;
            }
            if (q % 2u) CHECK(same);
            else CHECK(zero && rec[0] == 0 && rec[1] == 0 && rec[2] == 0 && rec[3] == 0 && rec[4] == (1u | 1u << 9) && rec[5] == 7u + q && rec[6] == 0 && rec[7] == 0);
        }
    CHECK(kmp_pack_regex_groups(mixed.data(), len.data(), flags.data(), gate.data(), N, 3, 1, 1, 1, 1, &grp, &ng, &msg) == KMPGPU_OK);
    CHECK(ng == KMP_RX_TILE + 1u && grp.size() == (size_t)((ng + KMP_RXG_TILE - 1u) / KMP_RXG_TILE) * KMP_RXG_TILE_WORDS);
    if (grp.size() >= KMP_RXG_TILE_WORDS) {
        /* the second flagged expression: q = 2, not gated, no $: accept bit 16 sticky in B and rep */
        const uint32_t *rec = grp.data() + 512u * KMP_RXG_TILE + 12u, *rule = grp.data() + 512u * KMP_RXG_TILE + 12u * KMP_RXG_TILE + 4u * KMPGPU_RX_MAX_EDGES;
        CHECK(rec[0] == 0 && rec[1] == 0 && rec[2] == 1u << 16 && rec[3] == 0 && rec[4] != 0 && rec[6] == (1u | 1u << 3 | 1u << 7 | 1u << 11) && rec[7] == 0);
        CHECK(rec[8] == (16u | 1u << 8 | 1u << 16) && rec[9] == 0 && rec[10] == 2 && rec[11] == 0);
        CHECK(rule[0] == (1u << 2 | 1u << 6 | 1u << 10) && rule[1] == 0 && rule[2] == 1u << 14 && rule[3] == 0 && rule[4] == 0);
        CHECK(grp[2u * ('G' * KMP_RXG_TILE + 1u)] == (1u | 1u << 16) && grp[2u * ('z' * KMP_RXG_TILE + 1u)] == 1u << 16);
        /* the first one is gated on pattern 2 */
        CHECK(grp[512u * KMP_RXG_TILE + 8u] == (16u | 1u << 8 | 1u << 9 | 1u << 16) && grp[512u * KMP_RXG_TILE + 9u] == 2 && grp[512u * KMP_RXG_TILE + 10u] == 0);
    }
    /* no flagged expression: no second table, and the first is what it was */
    CHECK(kmp_pack_regex_groups(alone.data(), len_alone.data(), nullptr, nullptr, N, 3, 1, 1, 1, 1, &grp, &ng, &msg) == KMPGPU_OK && ng == 0 && grp.empty());
    /* one call refuses a bad set: kmp_pack_regexes checks the flagged expressions too; bit 8 stays unknown */
    const char *b1 = "(a|)";
    const uint8_t *badx[2] = {(const uint8_t *)unflagged, (const uint8_t *)b1};
    const uint32_t blen[2] = {4, 4}, bflags[2] = {0, KMPGPU_RX_GROUPS}, b8[2] = {0, 8u | KMPGPU_RX_GROUPS}, noflag[2] = {0, 0};
    CHECK(refused(kmp_pack_regexes(badx, blen, bflags, nullptr, 2, 3, 0, 0, 0, 0, &got, &msg), msg, "kmpgpu_set_regexes: expression 1: position 3: an empty alternative"));
    CHECK(got.empty());
    CHECK(refused(kmp_pack_regex_groups(badx, blen, bflags, nullptr, 2, 3, 0, 0, 0, 0, &grp, &ng, &msg), msg, "kmpgpu_set_regexes: expression 1: position 3: an empty alternative"));
    CHECK(refused(kmp_pack_regexes(badx, blen, b8, nullptr, 2, 3, 0, 0, 0, 0, &got, &msg), msg, "kmpgpu_set_regexes: expression 1: unknown flag bits 0x8"));
    CHECK(refused(kmp_pack_regexes(badx, blen, noflag, nullptr, 2, 3, 0, 0, 0, 0, &got, &msg), msg,
                  "kmpgpu_set_regexes: expression 1: position 0: '(' is reserved: groups and alternation are not part of the dialect"));
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s <verdicts file>\n", argv[0]); return 2; }
    verdicts(argv[1]);
    refusals();
    tables();
    packers();
    if (g_failed) { fprintf(stderr, "%d checks failed\n", g_failed); return 1; }
    printf("regex groups driver ok\n");
    return 0;
}
