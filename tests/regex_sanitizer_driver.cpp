/* Built with -fsanitize=address,undefined by tests/test_regex_host.py: drives the compiler and the interpreter of csrc/kmp_regex.cpp,
 * kmp_pack_regexes and the n_rx entries of the other packers (csrc/kmp_rowtables.cpp), without a device.
 *   argv[1]: the verdicts file that the test wrote from tests/regex_model.py (Python's re):
 *       S <hex of a text, or - for the empty one>          the texts, once
 *       X <flags> <hex of an expression>                   an expression, then its two lines
 *       V <0 | 1: whole payloads> <one 0 / 1 per text>     the model's verdicts under either text-end rule
 * Every refusal's position and every packed word below is written out by hand from include/kmpgpu.h and csrc/kmp_regex.h. */
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

static int compile(const char *expr, size_t len, uint32_t flags, kmp_regex_table *t, std::string *msg)
{
    /* an exact-size heap copy: a read behind the expression is a finding */
    Bytes e(expr, expr + len);
    return kmp_regex_compile(e.data(), e.size(), flags, t, msg);
}

static bool search(const kmp_regex_table &t, const Bytes &text, size_t E)
{
    Bytes exact(text.begin(), text.begin() + E);          /* nothing at or behind E is the interpreter's to read */
    return kmp_regex_search(t, exact.data(), E);
}

/* the accepted expressions against the model's verdicts */
static void verdicts(const char *path)
{
    FILE *f = fopen(path, "r");
    CHECK(f != nullptr);
    if (!f) return;
    std::vector<Bytes> texts;
    std::vector<char> line(1 << 20);
    kmp_regex_table t;
    std::string msg;
    bool have = false;
    unsigned n_expr = 0;
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
            have = compile((const char *)e.data(), e.size(), flags, &t, &msg) == KMPGPU_OK;
            if (!have) fprintf(stderr, "expression %u (%s) refused: %s\n", n_expr, line.data(), msg.c_str());
            CHECK(have);
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
                const bool got = search(t, texts[i], E);
                n_verdicts++;
                if (got != (v[i] == '1') && wrong++ < 10)
                    fprintf(stderr, "expression %u, text %zu, whole %d: got %d, the model says %c\n", n_expr - 1, i, whole, (int)got, v[i]);
            }
        }
    }
    fclose(f);
    CHECK(wrong == 0);
    CHECK(n_expr >= 30 && texts.size() >= 2000);
    printf("%u expressions, %zu texts, %llu verdicts\n", n_expr, texts.size(), n_verdicts);
}

/* every refusal, with the position its message names */
static void refusals(void)
{
    static const struct { const char *expr; int len; uint32_t flags; const char *msg; } bad[] = {
        {"a(b", -1, 0, "position 1: '(' is reserved: groups and alternation are not part of the dialect"},
        {"ab)", -1, 0, "position 2: ')' is reserved: groups and alternation are not part of the dialect"},
        {"a|b", -1, 0, "position 1: '|' is reserved: groups and alternation are not part of the dialect"},
        {"*a", -1, 0, "position 0: a quantifier on nothing"},
        {"^+", -1, 0, "position 1: a quantifier on nothing"},
        {"{2}", -1, 0, "position 0: a quantifier on nothing"},
        {"a**", -1, 0, "position 2: a quantifier on a quantifier"},
        {"a+?", -1, 0, "position 2: a quantifier on a quantifier"},
        {"ab{2}{3}", -1, 0, "position 5: a quantifier on a quantifier"},
        {"a{,3}", -1, 0, "position 1: {,m} has no lower count"},
        {"a{3,2}", -1, 0, "position 1: {n,m} with n > m"},
        {"a{0}", -1, 0, "position 1: {n,m} needs m >= 1"},
        {"a{0,0}", -1, 0, "position 1: {n,m} needs m >= 1"},
        {"a{2", -1, 0, "position 1: unterminated brace"},
        {"a{2,", -1, 0, "position 1: unterminated brace"},
        {"a{2,3", -1, 0, "position 1: unterminated brace"},
        {"a{", -1, 0, "position 1: unterminated brace"},
        {"a{x}", -1, 0, "position 1: a brace without a count"},
        {"a{2x}", -1, 0, "position 1: a brace without a count"},
        {"a{2,3x}", -1, 0, "position 1: a brace without a count"},
        {"a}", -1, 0, "position 1: '}' without its opening (write \\})"},
        {"a]", -1, 0, "position 1: ']' without its opening (write \\])"},
        {"a^b", -1, 0, "position 1: '^' anywhere but first"},
        {"^^", -1, 0, "position 1: '^' anywhere but first"},
        {"a$b", -1, 0, "position 1: '$' anywhere but last"},
        {"$a", -1, 0, "position 0: '$' anywhere but last"},
        {"a\0b", 3, 0, "position 1: a raw 0x00 (write \\x00)"},
        {"[a\0]", 4, 0, "position 2: a raw 0x00 (write \\x00)"},
        {"[a-\0]", 5, 0, "position 3: a raw 0x00 (write \\x00)"},
        {"a\\q", -1, 0, "position 1: unknown escape \\q"},
        {"\\b", -1, 0, "position 0: unknown escape \\b"},
        {"a\\1", -1, 0, "position 1: unknown escape \\1"},
        {"[\\A]", -1, 0, "position 1: unknown escape \\A"},
        {"ab\\", -1, 0, "position 2: a backslash at the end of the expression"},
        {"\\x4", -1, 0, "position 0: \\x takes two hex digits"},
        {"a\\xg0", -1, 0, "position 1: \\x takes two hex digits"},
        {"\\01", -1, 0, "position 0: \\0 followed by a digit (octal escapes are not part of the dialect)"},
        {"[z-a]", -1, 0, "position 1: bad range: 0x7a lies above 0x61"},
        {"[a-\\d]", -1, 0, "position 1: bad range: a class escape is no endpoint"},
        {"[\\d-z]", -1, 0, "position 1: bad range: a class escape is no endpoint"},
        {"x[abc", -1, 0, "position 1: unterminated class"},
        {"[", -1, 0, "position 0: unterminated class"},
        {"[^", -1, 0, "position 0: unterminated class"},
        {"[a\\]", -1, 0, "position 0: unterminated class"},
        {"a[]", -1, 0, "position 1: empty class"},
        {"[^]", -1, 0, "position 0: empty class"},
        {"", 0, 0, "position 0: zero elements"},
        {"^", -1, 0, "position 1: zero elements"},
        {"$", -1, 0, "position 0: zero elements"},
        {"^$", -1, 0, "position 1: zero elements"},
        {"a{64}", -1, 0, "position 0: more than 63 positions"},
        {"a{63}b", -1, 0, "position 5: more than 63 positions"},
        {"ab{0,63}", -1, 0, "position 1: more than 63 positions"},
        {"a{99999999999}", -1, 0, "position 0: more than 63 positions"},
    };
    kmp_regex_table t;
    std::string msg;
    for (const auto &b : bad) {
        const size_t len = b.len < 0 ? strlen(b.expr) : (size_t)b.len;
        if (!refused(compile(b.expr, len, b.flags, &t, &msg), msg, b.msg)) { fprintf(stderr, "  (expression '%s')\n", b.expr); g_failed++; }
    }
}

static bool hit(const char *expr, uint32_t flags, const Bytes &text)
{
    kmp_regex_table t;
    std::string msg;
    if (compile(expr, strlen(expr), flags, &t, &msg)) { fprintf(stderr, "'%s' refused: %s\n", expr, msg.c_str()); g_failed++; return false; }
    return search(t, text, text.size());
}

/* the tables themselves, and the 63 positions */
static void tables(void)
{
    kmp_regex_table t;
    std::string msg;
    /* positions: a, b?, b?, [0-9]+, c*, d{2,}: 0 mandatory, 1 2 optional, 3 repeatable, 4 optional repeatable, 5 mandatory, 6 repeatable */
    CHECK(compile("^ab{0,2}\\d+c*d{2,}$", 19, 0, &t, &msg) == KMPGPU_OK);
    CHECK(t.n == 7 && t.bol && t.eol && t.opt == 0x16u && t.rep == 0x58u && t.opt_run == 2);
    CHECK(t.B['a'] == 0x01u && t.B['b'] == 0x06u && t.B['7'] == 0x08u && t.B['c'] == 0x10u && t.B['d'] == 0x60u && t.B['A'] == 0 && t.B[0] == 0);
    CHECK(compile("a[^b]", 5, KMPGPU_RX_NOCASE, &t, &msg) == KMPGPU_OK);
    CHECK(t.n == 2 && !t.bol && !t.eol && t.opt == 0 && t.rep == 0 && t.opt_run == 0);
    CHECK(t.B['a'] == 3u && t.B['A'] == 3u && t.B['b'] == 0 && t.B['B'] == 0 && t.B['\n'] == 2u && t.B[0] == 2u && t.B[255] == 2u);
    CHECK(compile(".x", 2, 0, &t, &msg) == KMPGPU_OK && t.B['\n'] == 0 && t.B[0] == 1u && t.B['x'] == 3u);
    CHECK(compile(".x", 2, KMPGPU_RX_DOTALL, &t, &msg) == KMPGPU_OK && t.B['\n'] == 1u);

    /* 63 positions: the match runs through accept bit 63 */
    CHECK(compile("a{63}", 5, 0, &t, &msg) == KMPGPU_OK && t.n == 63 && t.opt == 0 && t.rep == 0);
    CHECK(hit("a{63}", 0, Bytes(63, 'a')) && !hit("a{63}", 0, Bytes(62, 'a')) && hit("^a{63}$", 0, Bytes(63, 'a')) && !hit("^a{63}$", 0, Bytes(64, 'a')));
    Bytes far(70, 'b');
    for (int i = 3; i < 66; i++) far[i] = 'a';
    CHECK(hit("a{63}", 0, far));
    far[40] = 'b';
    CHECK(!hit("a{63}", 0, far));
    CHECK(compile(".{0,62}x", 8, 0, &t, &msg) == KMPGPU_OK && t.n == 63 && t.opt == 0x3FFFFFFFFFFFFFFFull && t.opt_run == 62);
    Bytes run(62, 'q');
    run.push_back('x');
    CHECK(hit(".{0,62}x", 0, Bytes(1, 'x')) && hit("^.{0,62}x$", 0, run) && !hit("^.{0,62}x$", 0, Bytes(63, 'q')));
    run.insert(run.begin(), 'q');
    CHECK(!hit("^.{0,62}x$", 0, run) && hit(".{0,62}x$", 0, run));
    CHECK(compile("a{62,}", 6, 0, &t, &msg) == KMPGPU_OK && t.n == 62 && t.rep == 1ull << 61);
    CHECK(compile("a{0,}", 5, 0, &t, &msg) == KMPGPU_OK && t.n == 1 && t.rep == 1 && t.opt == 1);
}

static void packer(void)
{
    const char *e0 = "ab+$", *e1 = "^[xy]";
    const uint8_t *expr[2] = {(const uint8_t *)e0, (const uint8_t *)e1};
    const uint32_t len[2] = {4, 5}, flags[2] = {0, KMPGPU_RX_GATED | KMPGPU_RX_NOCASE}, gate[2] = {0, 2};
    Words got;
    std::string msg;
    CHECK(kmp_pack_regexes(expr, len, flags, gate, 2, 3, 1, 1, 1, 1, &got, &msg) == KMPGPU_OK);
    CHECK(got.size() == KMP_RX_TILE_WORDS && KMP_RX_TILE_WORDS == 512u * KMP_RX_TILE + 8u * KMP_RX_TILE);
    /* the 64-bit word of (byte c, slot q) at 2 (c TILE + q); the records behind the 512 TILE words of B */
    auto B = [&](unsigned c, unsigned q) { return (uint64_t)got[2 * (c * KMP_RX_TILE + q) + 1] << 32 | got[2 * (c * KMP_RX_TILE + q)]; };
    const uint32_t *rec = got.data() + 512u * KMP_RX_TILE;
    if (got.size() == KMP_RX_TILE_WORDS) {
        /* "ab+$": positions a, b+; with $ nothing is sticky */
        CHECK(B('a', 0) == 1 && B('b', 0) == 2 && B('c', 0) == 0);
        CHECK(rec[0] == 0 && rec[1] == 0 && rec[2] == 2 && rec[3] == 0 && rec[4] == (2u | 1u << 8 | 1u << 10) && rec[5] == 0 && rec[6] == 0 && rec[7] == 0);
        /* "^[xy]" nocase, gated on pattern 2: one position, accept bit 1 sticky in every B word and in rep; no restart */
        CHECK(B('x', 1) == 3 && B('Y', 1) == 3 && B('z', 1) == 2 && B(0, 1) == 2);
        CHECK(rec[8] == 0 && rec[10] == 2 && rec[11] == 0 && rec[12] == (1u | 1u << 9) && rec[13] == 2);
        /* the empty slots are zero */
        CHECK(B('a', 2) == 0 && rec[16] == 0 && rec[20] == 0);
    }
    /* nine expressions: two tiles */
    const uint8_t *nine[9];
    uint32_t nlen[9];
    for (int i = 0; i < 9; i++) { nine[i] = (const uint8_t *)e0; nlen[i] = 4; }
    CHECK(kmp_pack_regexes(nine, nlen, nullptr, nullptr, KMP_RX_TILE + 1, 3, 0, 0, 0, 0, &got, &msg) == KMPGPU_OK && got.size() == 2u * KMP_RX_TILE_WORDS);

    /* every refusal; the table comes back empty */
    CHECK(refused(kmp_pack_regexes(nullptr, len, flags, gate, 2, 3, 0, 0, 0, 0, &got, &msg), msg, "kmpgpu_set_regexes: NULL expression arrays"));
    CHECK(got.empty());
    CHECK(refused(kmp_pack_regexes(expr, nullptr, flags, gate, 2, 3, 0, 0, 0, 0, &got, &msg), msg, "kmpgpu_set_regexes: NULL expression arrays"));
    uint32_t f2[2] = {0, 8};
    CHECK(refused(kmp_pack_regexes(expr, len, f2, gate, 2, 3, 0, 0, 0, 0, &got, &msg), msg, "kmpgpu_set_regexes: expression 1: unknown flag bits 0x8"));
    uint32_t g2[2] = {0, 3};
    CHECK(refused(kmp_pack_regexes(expr, len, flags, g2, 2, 3, 0, 0, 0, 0, &got, &msg), msg, "kmpgpu_set_regexes: expression 1: its gate names pattern 3 of 3"));
    g2[0] = 1; g2[1] = 2;
    CHECK(refused(kmp_pack_regexes(expr, len, flags, g2, 2, 3, 0, 0, 0, 0, &got, &msg), msg, "kmpgpu_set_regexes: expression 0 is not gated and names gate 1, not 0"));
    CHECK(refused(kmp_pack_regexes(expr, len, flags, nullptr, 2, 3, 0, 0, 0, 0, &got, &msg), msg, "kmpgpu_set_regexes: expression 1 is gated and gate is NULL"));
    const uint8_t *withnull[2] = {(const uint8_t *)e0, nullptr};
    CHECK(refused(kmp_pack_regexes(withnull, len, nullptr, nullptr, 2, 3, 0, 0, 0, 0, &got, &msg), msg, "kmpgpu_set_regexes: expression 1 is NULL"));
    const char *b1 = "a**";
    const uint8_t *badx[2] = {(const uint8_t *)e0, (const uint8_t *)b1};
    const uint32_t blen[2] = {4, 3};
    CHECK(refused(kmp_pack_regexes(badx, blen, nullptr, nullptr, 2, 3, 0, 0, 0, 0, &got, &msg), msg,
                  "kmpgpu_set_regexes: expression 1: position 2: a quantifier on a quantifier"));
    CHECK(got.empty());
    /* the 2^31 bound is checked on the counts alone, before an array is read */
    CHECK(refused(kmp_pack_regexes(expr, len, nullptr, nullptr, 0x7FFFFFF1u, 8, 2, 1, 3, 1, &got, &msg), msg,
                  "kmpgpu_set_regexes: 8 patterns + 2 relations + 1 chains + 3 header predicates + 1 byte tests + 2147483633 expressions do not fit the 2^31 rows a rule term can name"));
    CHECK(kmp_pack_regexes(expr, len, nullptr, nullptr, 2, 0x7FFFFFF9u, 1, 1, 1, 1, &got, &msg) == KMPGPU_OK);      /* 2^31 - 1 rows */
    CHECK(refused(kmp_pack_regexes(expr, len, nullptr, nullptr, 2, 0x7FFFFFFAu, 1, 1, 1, 1, &got, &msg), msg,
                  "kmpgpu_set_regexes: 2147483642 patterns + 1 relations + 1 chains + 1 header predicates + 1 byte tests + 2 expressions do not fit the 2^31 rows a rule term can name"));
}

/* the n_rx entries of the other packers: the rules' terms reach the expressions' rows, every 2^31 bound counts them in, and with
 * n_rx = 0 every message is what it was */
static void siblings(void)
{
    const uint32_t N = KMPGPU_RULE_NOT;
    /* 8 patterns + 1 relation + 1 chain + 2 predicates + 2 byte tests + 2 expressions = rows 0 .. 15 */
    const Words off = {0, 2, 3}, terms = {14, N | 15, N | 14};
    const Words want_heads = {0, 0, 14, N | 15,  0, 0, N | 14, N | 14};
    Words heads, quads;
    std::string msg;
    CHECK(kmp_pack_rules(off.data(), terms.data(), 2, 8, 1, 1, 2, 2, 2, &heads, &quads, &msg) == KMPGPU_OK);
    CHECK(heads == want_heads && quads.empty());
    CHECK(refused(kmp_pack_rules(off.data(), terms.data(), 2, 8, 1, 1, 2, 2, 1, &heads, &quads, &msg), msg,
                  "kmpgpu_set_rules: rule 0: term 1 names row 15 of 8 patterns + 1 relations + 1 chains + 2 header predicates + 2 byte tests + 1 expressions"));
    CHECK(refused(kmp_pack_rules(off.data(), terms.data(), 2, 8, 1, 1, 2, 2, 0, &heads, &quads, &msg), msg,
                  "kmpgpu_set_rules: rule 0: term 0 names row 14 of 8 patterns + 1 relations + 1 chains + 2 header predicates + 2 byte tests"));
    CHECK(refused(kmp_pack_rules(off.data(), terms.data(), 2, 8, 1, 1, 2, 2, &heads, &quads, &msg), msg,
                  "kmpgpu_set_rules: rule 0: term 0 names row 14 of 8 patterns + 1 relations + 1 chains + 2 header predicates + 2 byte tests"));
    CHECK(refused(kmp_pack_rules(off.data(), terms.data(), 2, 8, 1, 1, 2, 0, 0, &heads, &quads, &msg), msg,
                  "kmpgpu_set_rules: rule 0: term 0 names row 14 of 8 patterns + 1 relations + 1 chains + 2 header predicates"));
    CHECK(refused(kmp_pack_rules(off.data(), terms.data(), 2, 8, 1, 1, 0, 0, 0, &heads, &quads, &msg), msg,
                  "kmpgpu_set_rules: rule 0: term 0 names row 14 of 8 patterns + 1 relations + 1 chains"));

    const uint8_t fold[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const kmpgpu_relation rel = {1, 2, -3, 4};
    Words r;
    CHECK(kmp_pack_relations(&rel, 1, 8, 1, 5, 6, 7, fold, &r, &msg) == KMPGPU_OK && r == Words({1, 2, 0xFFFFFFFDu, 4}));
    CHECK(refused(kmp_pack_relations(&rel, 1, 8, 0, 0, 0, 0x7FFFFFF7u, fold, &r, &msg), msg,
                  "kmpgpu_set_relations: 8 patterns + 1 relations + the expressions do not fit the 2^31 rows a rule term can name"));
    CHECK(refused(kmp_pack_relations(&rel, 1, 8, 1, 1, 1, 0x7FFFFFF4u, fold, &r, &msg), msg,
                  "kmpgpu_set_relations: 8 patterns + 1 relations + the chains + the header predicates + the byte tests + the expressions do not fit the 2^31 rows a rule term can name"));
    CHECK(kmp_pack_relations(&rel, 1, 8, 0, 0, 0, 0x7FFFFFF6u, fold, &r, &msg) == KMPGPU_OK);
    CHECK(refused(kmp_pack_relations(&rel, 1, 8, 0, 0, 0x7FFFFFF7u, 0, fold, &r, &msg), msg,
                  "kmpgpu_set_relations: 8 patterns + 1 relations + the byte tests do not fit the 2^31 rows a rule term can name"));
    CHECK(refused(kmp_pack_relations(&rel, 1, 8, 0, 0, 0x7FFFFFF7u, fold, &r, &msg), msg,
                  "kmpgpu_set_relations: 8 patterns + 1 relations + the byte tests do not fit the 2^31 rows a rule term can name"));

    const Words coff = {0, 2};
    const kmpgpu_chain_link links[2] = {{1, INT32_MIN, INT32_MAX}, {2, 0, 5}};
    Words c;
    CHECK(kmp_pack_chains(coff.data(), links, 1, 8, 1, 3, 4, 5, fold, &c, &msg) == KMPGPU_OK && c.size() == 4u * KMPGPU_CHAIN_MAX);
    CHECK(refused(kmp_pack_chains(coff.data(), links, 1, 8, 1, 0, 0, 0x7FFFFFF6u, fold, &c, &msg), msg,
                  "kmpgpu_set_chains: 8 patterns + 1 relations + 1 chains + the expressions do not fit the 2^31 rows a rule term can name"));
    CHECK(kmp_pack_chains(coff.data(), links, 1, 8, 1, 0, 0, 0x7FFFFFF5u, fold, &c, &msg) == KMPGPU_OK);
    CHECK(refused(kmp_pack_chains(coff.data(), links, 1, 8, 1, 0, 0x7FFFFFF6u, 0, fold, &c, &msg), msg,
                  "kmpgpu_set_chains: 8 patterns + 1 relations + 1 chains + the byte tests do not fit the 2^31 rows a rule term can name"));

    kmpgpu_header h;
    memset(&h, 0, sizeof h);
    h.sport_hi = h.dport_hi = 0xFFFFu; h.len_hi = 0xFFFFFFFFu; h.flags = KMPGPU_HDR_ANY_PROTO;
    Words hw;
    CHECK(kmp_pack_headers(&h, 1, 8, 1, 1, 9, 9, &hw, &msg) == KMPGPU_OK && hw.size() == 12);
    CHECK(refused(kmp_pack_headers(&h, 1, 8, 2, 1, 1, 0x7FFFFFF3u, &hw, &msg), msg,
                  "kmpgpu_set_headers: 8 patterns + 2 relations + 1 chains + 1 header predicates + the byte tests + the expressions do not fit the 2^31 rows a rule term can name"));
    CHECK(kmp_pack_headers(&h, 1, 8, 2, 1, 1, 0x7FFFFFF2u, &hw, &msg) == KMPGPU_OK);
    CHECK(refused(kmp_pack_headers(&h, 1, 8, 2, 1, 0x7FFFFFF4u, 0, &hw, &msg), msg,
                  "kmpgpu_set_headers: 8 patterns + 2 relations + 1 chains + 1 header predicates + the byte tests do not fit the 2^31 rows a rule term can name"));

    kmpgpu_bytetest b;
    memset(&b, 0, sizeof b);
    b.nbytes = 2; b.mask = 0xFFFFFFFFu;
    Words bw;
    uint32_t n_rel = 0, reach = 0;
    CHECK(kmp_pack_bytetests(&b, 1, 8, 1, 1, 1, 5, fold, &bw, &n_rel, &reach, &msg) == KMPGPU_OK && bw.size() == 8 && reach == 2);
    CHECK(refused(kmp_pack_bytetests(&b, 1, 8, 2, 1, 3, 0x7FFFFFF1u, fold, &bw, &n_rel, &reach, &msg), msg,
                  "kmpgpu_set_bytetests: 8 patterns + 2 relations + 1 chains + 3 header predicates + 1 byte tests + the expressions do not fit the 2^31 rows a rule term can name"));
    CHECK(kmp_pack_bytetests(&b, 1, 8, 2, 1, 3, 0x7FFFFFF0u, fold, &bw, &n_rel, &reach, &msg) == KMPGPU_OK);
    CHECK(refused(kmp_pack_bytetests(&b, 0x7FFFFFF2u, 8, 2, 1, 3, 0, fold, &bw, &n_rel, &reach, &msg), msg,
                  "kmpgpu_set_bytetests: 8 patterns + 2 relations + 1 chains + 3 header predicates + 2147483634 byte tests do not fit the 2^31 rows a rule term can name"));
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s <verdicts file>\n", argv[0]); return 2; }
    verdicts(argv[1]);
    refusals();
    tables();
    packer();
    siblings();
    if (g_failed) { fprintf(stderr, "%d checks failed\n", g_failed); return 1; }
    printf("regex driver ok\n");
    return 0;
}
