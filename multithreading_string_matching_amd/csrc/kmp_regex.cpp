/*
 * kmp_regex.cpp -- the compiler and the host interpreter of the expressions of kmpgpu_set_regexes (kmp_regex.h).  Host code only.
 */
#include "kmp_regex.h"

#include "kmp_rowtables.h"

#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <bitset>
#include <vector>

namespace {

typedef std::bitset<256> ByteSet;

struct Position {
    ByteSet cls;
    bool opt, rep;
};

struct Parser {
    const uint8_t *e;
    size_t len, pos;
    uint32_t flags;
    std::string *msg;
};

int refuse_at(Parser *p, size_t at, const char *fmt, ...)
{
    char what[192], buf[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(what, sizeof what, fmt, ap);
    va_end(ap);
    snprintf(buf, sizeof buf, "position %zu: %s", at, what);
    if (p->msg) *p->msg = buf;
    return KMPGPU_EINVAL;
}

bool is_digit(uint8_t c) { return c >= '0' && c <= '9'; }
bool is_alpha(uint8_t c) { return (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z'); }
bool is_punct(uint8_t c) { return c > 0x20 && c < 0x7F && !is_digit(c) && !is_alpha(c); }
int  hex_digit(uint8_t c) { return is_digit(c) ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1; }

void add_range(ByteSet *s, unsigned lo, unsigned hi) { for (unsigned c = lo; c <= hi; c++) s->set(c); }

/* the listed set closed under ASCII case (KMPGPU_RX_NOCASE: before a [^...] negates it) */
void close_case(ByteSet *s)
{
    for (unsigned c = 'a'; c <= 'z'; c++)
        if (s->test(c) || s->test(c - 32u)) { s->set(c); s->set(c - 32u); }
}

/* \d \D \w \W \s \S in Python's ASCII meaning on bytes */
bool class_escape(uint8_t letter, ByteSet *s)
{
    ByteSet t;
    switch (letter | 0x20) {
    case 'd': add_range(&t, '0', '9'); break;
    case 'w': add_range(&t, '0', '9'); add_range(&t, 'a', 'z'); add_range(&t, 'A', 'Z'); t.set('_'); break;
    case 's': add_range(&t, 9, 13); t.set(32); break;
    default: return false;
    }
    if (!(letter & 0x20)) t.flip();
    *s |= t;
    return true;
}

/* The escape whose backslash is at p->pos: 1 with *byte, 2 with a class escape's set added to *cls, or the refusal (< 0). */
int escape(Parser *p, uint8_t *byte, ByteSet *cls)
{
    const size_t at = p->pos;
    if (at + 1 >= p->len) return refuse_at(p, at, "a backslash at the end of the expression");
    const uint8_t c = p->e[at + 1];
    p->pos = at + 2;
    if (c == 'x') {
        const int h = at + 2 < p->len ? hex_digit(p->e[at + 2]) : -1, l = at + 3 < p->len ? hex_digit(p->e[at + 3]) : -1;
        if (h < 0 || l < 0) return refuse_at(p, at, "\\x takes two hex digits");
        *byte = (uint8_t)(h * 16 + l);
        p->pos = at + 4;
        return 1;
    }
    switch (c) {
    case 'n': *byte = '\n'; return 1;
    case 'r': *byte = '\r'; return 1;
    case 't': *byte = '\t'; return 1;
    case 'f': *byte = '\f'; return 1;
    case 'v': *byte = '\v'; return 1;
    case '0':
        if (at + 2 < p->len && is_digit(p->e[at + 2])) return refuse_at(p, at, "\\0 followed by a digit (octal escapes are not part of the dialect)");
        *byte = 0;
        return 1;
    default: break;
    }
    if (class_escape(c, cls) ) return 2;
    if (is_punct(c)) { *byte = c; return 1; }
    if (c >= 0x20 && c < 0x7F) return refuse_at(p, at, "unknown escape \\%c", c);
    return refuse_at(p, at, "unknown escape \\ 0x%02x", c);
}

/* [...] whose bracket is at p->pos */
int bracket(Parser *p, ByteSet *out)
{
    const size_t open = p->pos;
    size_t i = open + 1;
    bool negate = false;
    if (i < p->len && p->e[i] == '^') { negate = true; i++; }
    ByteSet s;
    bool any = false;
    for (;;) {
        if (i >= p->len) return refuse_at(p, open, "unterminated class");
        const uint8_t c = p->e[i];
        if (c == ']') { i++; break; }
        /* one item: a byte, or a class escape */
        const size_t item_at = i;
        uint8_t lo = c;
        int kind = 1;
        if (c == 0) return refuse_at(p, i, "a raw 0x00 (write \\x00)");
        if (c == '\\') {
            p->pos = i;
            kind = escape(p, &lo, &s);
            if (kind < 0) return kind;
            i = p->pos;
        } else
            i++;
        any = true;
        /* a range?  a '-' that is first, last or escaped is a literal: it is an item itself, or has no endpoint behind it */
        const bool dash = i + 1 < p->len && p->e[i] == '-' && p->e[i + 1] != ']';
        if (!dash) {
            if (kind == 1) s.set(lo);
            continue;
        }
        if (kind == 2) return refuse_at(p, item_at, "bad range: a class escape is no endpoint");
        i++;                                               /* the '-' */
        uint8_t hi = p->e[i];
        if (hi == 0) return refuse_at(p, i, "a raw 0x00 (write \\x00)");
        if (hi == '\\') {
            ByteSet none;
            p->pos = i;
            const int k2 = escape(p, &hi, &none);
            if (k2 < 0) return k2;
            if (k2 == 2) return refuse_at(p, item_at, "bad range: a class escape is no endpoint");
            i = p->pos;
        } else
            i++;
        if (hi < lo) return refuse_at(p, item_at, "bad range: 0x%02x lies above 0x%02x", lo, hi);
        add_range(&s, lo, hi);
    }
    if (!any) return refuse_at(p, open, "empty class");
    if (p->flags & KMPGPU_RX_NOCASE) close_case(&s);
    if (negate) s.flip();
    *out = s;
    p->pos = i;
    return KMPGPU_OK;
}

/* a decimal count at p->pos, capped far above any that fits; false where there is no digit */
bool count(Parser *p, uint32_t *v)
{
    const size_t at = p->pos;
    uint32_t n = 0;
    while (p->pos < p->len && is_digit(p->e[p->pos])) {
        if (n < 100000u) n = n * 10u + (uint32_t)(p->e[p->pos] - '0');
        p->pos++;
    }
    *v = n;
    return p->pos > at;
}

/* one element at p->pos -- an escape, the dot, a bracket class or a literal byte (the metacharacters are the caller's) -- as its class */
int element(Parser *p, ByteSet *cls)
{
    const uint8_t c = p->e[p->pos];
    if (c == '\\') {
        uint8_t b = 0;
        const int kind = escape(p, &b, cls);
        if (kind < 0) return kind;
        if (kind == 1) cls->set(b);
        if (p->flags & KMPGPU_RX_NOCASE) close_case(cls);
    } else if (c == '.') {
        cls->set();
        if (!(p->flags & KMPGPU_RX_DOTALL)) cls->reset('\n');
        p->pos++;
    } else if (c == '[') {
        const int rc = bracket(p, cls);
        if (rc) return rc;
    } else {
        cls->set(c);
        if (p->flags & KMPGPU_RX_NOCASE) close_case(cls);
        p->pos++;
    }
    return KMPGPU_OK;
}

/* the quantifier at p->pos, if there is one: *mand mandatory copies, *opt optional ones, *rep: the last mandatory one repeats, or the
 * only optional one (C*, C{0,}) */
int quantifier(Parser *p, uint32_t *mand, uint32_t *opt, bool *rep)
{
    const uint8_t *expr = p->e;
    const size_t len = p->len, qat = p->pos;
    const uint8_t q = qat < len ? expr[qat] : 0;
    *mand = 1; *opt = 0; *rep = false;
    if (q == '?') { *mand = 0; *opt = 1; p->pos++; }
    else if (q == '*') { *mand = 0; *opt = 1; *rep = true; p->pos++; }
    else if (q == '+') { *rep = true; p->pos++; }
    else if (q == '{') {
        p->pos++;
        uint32_t n = 0, m = 0;
        if (p->pos < len && expr[p->pos] == ',') return refuse_at(p, qat, "{,m} has no lower count");
        if (!count(p, &n)) return refuse_at(p, qat, p->pos < len ? "a brace without a count" : "unterminated brace");
        if (p->pos >= len) return refuse_at(p, qat, "unterminated brace");
        if (expr[p->pos] == '}') {
            if (n < 1) return refuse_at(p, qat, "{n,m} needs m >= 1");
            *mand = n;
        } else if (expr[p->pos] == ',') {
            p->pos++;
            if (p->pos >= len) return refuse_at(p, qat, "unterminated brace");
            if (expr[p->pos] == '}') {                 /* {n,} */
                *rep = true;
                if (n == 0) { *mand = 0; *opt = 1; } else *mand = n;
            } else {
                if (!count(p, &m)) return refuse_at(p, qat, "a brace without a count");
                if (p->pos >= len) return refuse_at(p, qat, "unterminated brace");
                if (expr[p->pos] != '}') return refuse_at(p, qat, "a brace without a count");
                if (n > m) return refuse_at(p, qat, "{n,m} with n > m");
                if (m < 1) return refuse_at(p, qat, "{n,m} needs m >= 1");
                *mand = n; *opt = m - n;
            }
        } else
            return refuse_at(p, qat, "a brace without a count");
        p->pos++;                                      /* the '}' */
    }
    if (p->pos > qat && p->pos < len && (expr[p->pos] == '*' || expr[p->pos] == '+' || expr[p->pos] == '?' || expr[p->pos] == '{'))
        return refuse_at(p, p->pos, "a quantifier on a quantifier");
    return KMPGPU_OK;
}

}  // namespace

int kmp_regex_compile(const uint8_t *expr, size_t len, uint32_t flags, kmp_regex_table *table, std::string *msg)
{
    Parser P = {expr, len, 0, flags, msg}, *p = &P;
    if (msg) msg->clear();
    if (!expr && len) return refuse_at(p, 0, "the expression is NULL");
    std::vector<Position> seq;
    bool bol = false, eol = false;
    if (len && expr[0] == '^') { bol = true; p->pos = 1; }
    while (p->pos < len) {
        const size_t at = p->pos;
        const uint8_t c = expr[at];
        ByteSet cls;
        if (c == '$') {
            if (at + 1 != len) return refuse_at(p, at, "'$' anywhere but last");
            eol = true;
            p->pos++;
            break;
        }
        if (c == '^') return refuse_at(p, at, "'^' anywhere but first");
        if (c == '(' || c == ')' || c == '|') return refuse_at(p, at, "'%c' is reserved: groups and alternation are not part of the dialect", c);
        if (c == '*' || c == '+' || c == '?' || c == '{') return refuse_at(p, at, "a quantifier on nothing");
        if (c == ']' || c == '}') return refuse_at(p, at, "'%c' without its opening (write \\%c)", c, c);
        if (c == 0) return refuse_at(p, at, "a raw 0x00 (write \\x00)");
        const int er = element(p, &cls);
        if (er) return er;
        /* the quantifier: mandatory positions, optional ones, and whether the last one repeats */
        uint32_t mand = 1, opt = 0;
        bool rep = false;
        const int qr = quantifier(p, &mand, &opt, &rep);
        if (qr) return qr;
        if (seq.size() + mand + opt > KMPGPU_RX_MAX_POSITIONS)
            return refuse_at(p, at, "more than %d positions", KMPGPU_RX_MAX_POSITIONS);
        /* the repeatable position is the last mandatory one, or the only optional one (C*, C{0,}) */
        for (uint32_t i = 0; i < mand; i++) seq.push_back({cls, false, rep && i + 1 == mand});
        for (uint32_t i = 0; i < opt; i++) seq.push_back({cls, true, rep && mand == 0});
    }
    if (seq.empty()) return refuse_at(p, bol ? 1 : 0, "zero elements");

    memset(table, 0, sizeof *table);
    table->n = (uint32_t)seq.size();
    table->bol = bol; table->eol = eol;
    uint32_t run = 0;
    for (uint32_t i = 0; i < table->n; i++) {
        for (unsigned c = 0; c < 256; c++)
            if (seq[i].cls.test(c)) table->B[c] |= 1ull << i;
        if (seq[i].opt) table->opt |= 1ull << i;
        if (seq[i].rep) table->rep |= 1ull << i;
        run = seq[i].opt ? run + 1 : 0;
        if (run > table->opt_run) table->opt_run = run;
    }
    return KMPGPU_OK;
}

namespace {

/* every position reachable from X by passing over optional ones */
uint64_t closure(uint64_t X, uint64_t opt, uint32_t opt_run)
{
    for (uint32_t i = 0; i < opt_run; i++) X |= (X & opt) << 1;
    return X;
}

}  // namespace

bool kmp_regex_search(const kmp_regex_table &t, const uint8_t *text, size_t E)
{
    uint64_t R = closure(1ull, t.opt, t.opt_run);
    bool hit = ((R >> t.n) & 1ull) && (!t.eol || E == 0);
    for (size_t i = 0; i < E && !hit; i++) {
        const uint64_t b = R & t.B[text[i]];
        uint64_t N = b << 1 | (b & t.rep);
        if (!t.bol) N |= 1ull;
        R = closure(N, t.opt, t.opt_run);
        if (((R >> t.n) & 1ull) && (!t.eol || i == E - 1)) hit = true;
    }
    return hit;
}

/* ---- KMPGPU_RX_GROUPS: the expression as a tree, unrolled, and its Glushkov automaton (kmp_regex.h) ---- */

namespace {

struct Node {
    enum Kind { LEAF, CAT, ALT, OPT, PLUS } kind;
    ByteSet cls;                       /* LEAF */
    std::vector<Node> kids;            /* CAT, ALT: two or more; OPT, PLUS: one */
    uint32_t npos;                     /* leaves below */
};

Node wrap(Node::Kind kind, const Node &g)
{
    Node n = {kind, ByteSet(), {g}, g.npos};
    return n;
}

/* CAT or ALT of kids, or the only one itself */
Node join(Node::Kind kind, std::vector<Node> *kids)
{
    if (kids->size() == 1) return (*kids)[0];
    Node n = {kind, ByteSet(), {}, 0};
    for (const Node &k : *kids) n.npos += k.npos;
    n.kids.swap(*kids);
    return n;
}

struct GroupParser {
    Parser P;
    bool eol;
    size_t bar;                        /* the first top-level |, or SIZE_MAX */
};

int parse_alt(GroupParser *g, uint32_t depth, size_t open, Node *out);

/* A run of quantified elements and groups up to the end, a | or a ).  base: the positions of the alternatives in front of it, which count
 * against the budget with its own.  Zero items: out->npos == 0, and the caller says what that is. */
int parse_seq(GroupParser *g, uint32_t depth, uint32_t base, Node *out)
{
    Parser *p = &g->P;
    std::vector<Node> items;
    uint32_t used = base;
    out->npos = 0;
    while (p->pos < p->len) {
        const size_t at = p->pos;
        const uint8_t c = p->e[at];
        if (c == '|' || c == ')') break;
        if (c == '$') {
            if (at + 1 != p->len) return refuse_at(p, at, "'$' anywhere but last");
            g->eol = true;
            p->pos++;
            break;
        }
        if (c == '^') return refuse_at(p, at, "'^' anywhere but first");
        if (c == '*' || c == '+' || c == '?' || c == '{') return refuse_at(p, at, "a quantifier on nothing");
        if (c == ']' || c == '}') return refuse_at(p, at, "'%c' without its opening (write \\%c)", c, c);
        if (c == 0) return refuse_at(p, at, "a raw 0x00 (write \\x00)");
        Node atom = {Node::LEAF, ByteSet(), {}, 1};
        if (c == '(') {
            if (depth + 1 > KMP_RXG_MAX_DEPTH) return refuse_at(p, at, "groups nested deeper than %d", KMP_RXG_MAX_DEPTH);
            p->pos++;
            if (p->pos < p->len && p->e[p->pos] == '?') {
                if (p->pos + 1 >= p->len || p->e[p->pos + 1] != ':')
                    return refuse_at(p, at, "'(?' opens no group but (?: ... ): look-around, names and inline flags are not part of the dialect");
                p->pos += 2;
            }
            const int rc = parse_alt(g, depth + 1, at, &atom);
            if (rc) return rc;
            if (p->pos >= p->len || p->e[p->pos] != ')') return refuse_at(p, at, "unterminated group");
            p->pos++;
        } else {
            const int er = element(p, &atom.cls);
            if (er) return er;
        }
        uint32_t mand = 1, opt = 0;
        bool rep = false;
        const int qr = quantifier(p, &mand, &opt, &rep);
        if (qr) return qr;
        /* (counts are capped at 100000 and npos at 63: the product fits) */
        if ((uint64_t)used + (uint64_t)atom.npos * (mand + opt) > KMPGPU_RX_MAX_POSITIONS)
            return refuse_at(p, at, "more than %d positions", KMPGPU_RX_MAX_POSITIONS);
        used += atom.npos * (mand + opt);
        /* unrolled: the repeating copy is the last mandatory one, or the only optional one (G*, G{0,}) */
        for (uint32_t i = 0; i < mand; i++) items.push_back(rep && i + 1 == mand ? wrap(Node::PLUS, atom) : atom);
        for (uint32_t i = 0; i < opt; i++) items.push_back(wrap(Node::OPT, rep && mand == 0 ? wrap(Node::PLUS, atom) : atom));
    }
    if (!items.empty()) *out = join(Node::CAT, &items);
    return KMPGPU_OK;
}

/* alternatives up to the end or the ) of the group opened at `open` (depth > 0) */
int parse_alt(GroupParser *g, uint32_t depth, size_t open, Node *out)
{
    Parser *p = &g->P;
    std::vector<Node> alts;
    uint32_t used = 0;
    for (;;) {
        Node seq;
        const int rc = parse_seq(g, depth, used, &seq);
        if (rc) return rc;
        const bool bar = p->pos < p->len && p->e[p->pos] == '|';
        if (seq.npos == 0) {
            if (depth && alts.empty() && p->pos < p->len && p->e[p->pos] == ')') return refuse_at(p, open, "an empty group");
            if (!depth && alts.empty() && !bar && (p->pos >= p->len || p->e[p->pos] != ')')) return refuse_at(p, open, "zero elements");
            if (alts.empty() && !bar && depth) return refuse_at(p, open, "unterminated group");
            if (bar || !alts.empty()) return refuse_at(p, p->pos, "an empty alternative");
        }
        if (!depth && p->pos < p->len && p->e[p->pos] == ')') return refuse_at(p, p->pos, "')' without its opening (write \\))");
        used += seq.npos;
        alts.push_back(seq);
        if (!bar) break;
        if (!depth && g->bar == SIZE_MAX) g->bar = p->pos;
        p->pos++;
    }
    *out = join(Node::ALT, &alts);
    return KMPGPU_OK;
}

struct Glushkov {
    uint64_t F[KMPGPU_RX_MAX_POSITIONS];       /* follow(j), bit n not yet in */
    ByteSet cls[KMPGPU_RX_MAX_POSITIONS];
    uint32_t n;
};

struct Sets {
    bool nullable;
    uint64_t first, last;
};

void link(Glushkov *a, uint64_t from, uint64_t to)
{
    for (uint32_t j = 0; j < a->n; j++)
        if ((from >> j) & 1ull) a->F[j] |= to;
}

/* numbers the leaves below node left to right and adds the follow sets it gives rise to */
Sets glushkov(const Node &node, Glushkov *a)
{
    if (node.kind == Node::LEAF) {
        const uint64_t bit = 1ull << a->n;
        a->cls[a->n] = node.cls;
        a->F[a->n++] = 0;
        return {false, bit, bit};
    }
    Sets s = glushkov(node.kids[0], a);
    if (node.kind == Node::OPT) s.nullable = true;
    if (node.kind == Node::PLUS) link(a, s.last, s.first);
    for (size_t i = 1; i < node.kids.size(); i++) {
        const Sets k = glushkov(node.kids[i], a);
        if (node.kind == Node::ALT) {
            s.nullable = s.nullable || k.nullable; s.first |= k.first; s.last |= k.last;
        } else {
            link(a, s.last, k.first);
            s.first |= s.nullable ? k.first : 0ull;
            s.last = k.last | (k.nullable ? s.last : 0ull);
            s.nullable = s.nullable && k.nullable;
        }
    }
    return s;
}

/* every position reachable from N by passing over optional ones: adding the optional positions of N to opt carries through each run of
 * optional positions up to the first position behind it (what the kernels compute) */
uint64_t carry_closure(uint64_t N, uint64_t opt) { return N | ((opt + (N & opt)) ^ opt); }

}  // namespace

int kmp_regex_compile_groups(const uint8_t *expr, size_t len, uint32_t flags, kmp_regex_groups_table *table, std::string *msg)
{
    GroupParser G = {{expr, len, 0, flags, msg}, false, SIZE_MAX};
    Parser *p = &G.P;
    if (msg) msg->clear();
    if (!expr && len) return refuse_at(p, 0, "the expression is NULL");
    const bool bol = len && expr[0] == '^';
    if (bol) p->pos = 1;
    Node root;
    const int rc = parse_alt(&G, 0, p->pos, &root);
    if (rc) return rc;
    if (G.bar != SIZE_MAX && (bol || G.eol))
        return refuse_at(p, G.bar, "a top-level '|' beside ^ or $ (write ^(a|b)$: the anchors hold for the whole expression)");

    Glushkov a;
    a.n = 0;
    const Sets s = glushkov(root, &a);
    const uint32_t n = a.n;
    const uint64_t accept = 1ull << n;
    for (uint32_t j = 0; j < n; j++)
        if ((s.last >> j) & 1ull) a.F[j] |= accept;
    const uint64_t first = s.first | (s.nullable ? accept : 0ull);

    memset(table, 0, sizeof *table);
    table->n = n;
    table->bol = bol; table->eol = G.eol;
    table->first = first;
    for (uint32_t i = 0; i < n; i++) {
        for (unsigned c = 0; c < 256; c++)
            if (a.cls[i].test(c)) table->B[c] |= 1ull << i;
        const uint64_t bit = 1ull << i;
        if (a.F[i] & bit) table->rep |= bit;
        if (a.F[i] & bit << 1) table->shift |= bit;
        bool opt = !(first & bit) || (first & bit << 1);
        for (uint32_t j = 0; j < n && opt; j++) opt = !(a.F[j] & bit) || (a.F[j] & bit << 1);
        if (opt) table->opt |= bit;
    }
    /* The rules: what the shift, the repeat and the closure leave of each follow set.  The two "internal:" refusals below are the
     * self-check kmp_regex.h promises, and no expression reaches them.  closure() of a subset of F(j) stays inside F(j), because a member
     * of OPT that is in F(j) has its right neighbour in F(j) by OPT's definition; and it reaches all of F(j), because each member t is in
     * the closure of the seed, or in T, or has t - 1 in F(j) and in OPT -- and then t - 1 is reached by induction and the closure steps
     * from it onto t.  FIRST is closed by the second clause of OPT's definition.  They are kept so that a mistake in a later change to
     * the derivation is a refused expression and not a wrong row. */
    std::vector<uint64_t> src, dst;
    for (uint32_t j = 0; j < n; j++) {
        const uint64_t bit = 1ull << j, seed = ((table->shift & bit) << 1) | (table->rep & bit);
        const uint64_t T = a.F[j] & ~carry_closure(seed, table->opt) & ~((a.F[j] & table->opt) << 1);
        if (carry_closure(seed | T, table->opt) != a.F[j]) return refuse_at(p, 0, "internal: the follow set of position %u is not closed", j);
        if (!T) continue;
        size_t r = 0;
        while (r < dst.size() && dst[r] != T) r++;
        if (r == dst.size()) { src.push_back(0); dst.push_back(T); }
        src[r] |= bit;
    }
    if (dst.size() > KMPGPU_RX_MAX_EDGES) return refuse_at(p, 0, "needs %zu edge rules, more than %d", dst.size(), KMPGPU_RX_MAX_EDGES);
    if (carry_closure(first, table->opt) != first) return refuse_at(p, 0, "internal: FIRST is not closed");
    table->n_rules = (uint32_t)dst.size();
    for (size_t r = 0; r < dst.size(); r++) { table->src[r] = src[r]; table->dst[r] = dst[r]; }
    return KMPGPU_OK;
}

bool kmp_regex_search_groups(const kmp_regex_groups_table &t, const uint8_t *text, size_t E)
{
    const uint64_t restart = t.bol ? 0ull : t.first;
    uint64_t R = t.first;
    bool hit = ((R >> t.n) & 1ull) && (!t.eol || E == 0);
    for (size_t i = 0; i < E && !hit; i++) {
        const uint64_t b = R & t.B[text[i]];
        uint64_t N = (b & t.shift) << 1 | (b & t.rep);
        for (uint32_t r = 0; r < t.n_rules; r++)
            if (b & t.src[r]) N |= t.dst[r];
        R = carry_closure(N, t.opt) | restart;
        if (((R >> t.n) & 1ull) && (!t.eol || i == E - 1)) hit = true;
    }
    return hit;
}

/* ---- kmp_pack_regexes (kmp_rowtables.h): here and not in kmp_rowtables.cpp, which links without the compiler ---- */

namespace {

int refuse_pack(std::string *msg, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    *msg = buf;
    return KMPGPU_EINVAL;
}

}  // namespace

namespace {

/* what both packers ask of expression q before they compile it */
int check_expression(const uint8_t *const *expr, const uint32_t *flags, const uint32_t *gate, uint32_t q, uint32_t n_pat, std::string *msg)
{
    const uint32_t known = KMPGPU_RX_NOCASE | KMPGPU_RX_DOTALL | KMPGPU_RX_GATED | KMPGPU_RX_GROUPS;
    const uint32_t f = flags ? flags[q] : 0u, g = gate ? gate[q] : 0u;
    if (f & ~known) return refuse_pack(msg, "kmpgpu_set_regexes: expression %u: unknown flag bits 0x%x", q, f & ~known);
    if ((f & KMPGPU_RX_GATED) && !gate) return refuse_pack(msg, "kmpgpu_set_regexes: expression %u is gated and gate is NULL", q);
    if ((f & KMPGPU_RX_GATED) && g >= n_pat) return refuse_pack(msg, "kmpgpu_set_regexes: expression %u: its gate names pattern %u of %u", q, g, n_pat);
    if (!(f & KMPGPU_RX_GATED) && g != 0) return refuse_pack(msg, "kmpgpu_set_regexes: expression %u is not gated and names gate %u, not 0", q, g);
    if (!expr[q]) return refuse_pack(msg, "kmpgpu_set_regexes: expression %u is NULL", q);
    return KMPGPU_OK;
}

int check_arrays(const uint8_t *const *expr, const uint32_t *expr_len, uint32_t n_rx, uint32_t n_pat, uint32_t n_rel, uint32_t n_chains,
                 uint32_t n_hdr, uint32_t n_bt, std::string *msg)
{
    if (!expr || !expr_len) return refuse_pack(msg, "kmpgpu_set_regexes: NULL expression arrays");
    if ((uint64_t)n_pat + n_rel + n_chains + n_hdr + n_bt + n_rx >= (1ull << 31))
        return refuse_pack(msg, "kmpgpu_set_regexes: %u patterns + %u relations + %u chains + %u header predicates + %u byte tests + %u expressions do not fit the 2^31 rows a rule term can name",
                      n_pat, n_rel, n_chains, n_hdr, n_bt, n_rx);
    return KMPGPU_OK;
}

void put64(uint32_t *w, uint64_t v) { w[0] = (uint32_t)v; w[1] = (uint32_t)(v >> 32); }

}  // namespace

int kmp_pack_regexes(const uint8_t *const *expr, const uint32_t *expr_len, const uint32_t *flags, const uint32_t *gate, uint32_t n_rx,
                     uint32_t n_pat, uint32_t n_rel, uint32_t n_chains, uint32_t n_hdr, uint32_t n_bt, std::vector<uint32_t> *tables,
                     std::string *msg)
{
    tables->clear();
    const int ca = check_arrays(expr, expr_len, n_rx, n_pat, n_rel, n_chains, n_hdr, n_bt, msg);
    if (ca) return ca;
    const uint32_t tiles = (n_rx + KMP_RX_TILE - 1u) / KMP_RX_TILE;
    std::vector<uint32_t> out((size_t)tiles * KMP_RX_TILE_WORDS, 0u);      /* a refusal leaves *tables empty */
    kmp_regex_table t;
    kmp_regex_groups_table tg;
    std::string why;
    for (uint32_t q = 0; q < n_rx; q++) {
        const uint32_t f = flags ? flags[q] : 0u, g = gate ? gate[q] : 0u;
        const int ce = check_expression(expr, flags, gate, q, n_pat, msg);
        if (ce) return ce;
        uint32_t *tile = out.data() + (size_t)(q / KMP_RX_TILE) * KMP_RX_TILE_WORDS;
        const uint32_t qi = q % KMP_RX_TILE;
        uint32_t *rec = tile + 512u * KMP_RX_TILE + 8u * qi;
        if (f & KMPGPU_RX_GROUPS) {
            /* kmp_pack_regex_groups' to lay out; here it is checked, and its slot holds one position that no byte takes, gated on the
             * expression's own row: the marking pass has zeroed that row, so no lane is active for it and the kernel stores zeros there */
            if (kmp_regex_compile_groups(expr[q], expr_len[q], f, &tg, &why)) return refuse_pack(msg, "kmpgpu_set_regexes: expression %u: %s", q, why.c_str());
            rec[4] = 1u | 1u << 9;
            rec[5] = n_pat + n_rel + n_chains + n_hdr + n_bt + q;
            continue;
        }
        if (kmp_regex_compile(expr[q], expr_len[q], f, &t, &why)) return refuse_pack(msg, "kmpgpu_set_regexes: expression %u: %s", q, why.c_str());
        /* an expression without $ stays accepted: its accept bit n loops on every byte */
        const uint64_t sticky = t.eol ? 0ull : 1ull << t.n;
        for (uint32_t c = 0; c < 256u; c++) put64(tile + 2u * (c * KMP_RX_TILE + qi), t.B[c] | sticky);
        put64(rec, t.opt);
        put64(rec + 2, t.rep | sticky);
        rec[4] = t.n | (t.bol ? 0u : 1u << 8) | ((f & KMPGPU_RX_GATED) ? 1u << 9 : 0u) | (t.eol ? 1u << 10 : 0u) | t.opt_run << 16;
        rec[5] = g;
    }
    tables->swap(out);
    return KMPGPU_OK;
}

int kmp_pack_regex_groups(const uint8_t *const *expr, const uint32_t *expr_len, const uint32_t *flags, const uint32_t *gate, uint32_t n_rx,
                          uint32_t n_pat, uint32_t n_rel, uint32_t n_chains, uint32_t n_hdr, uint32_t n_bt, std::vector<uint32_t> *tables,
                          uint32_t *n_groups, std::string *msg)
{
    tables->clear();
    *n_groups = 0;
    const int ca = check_arrays(expr, expr_len, n_rx, n_pat, n_rel, n_chains, n_hdr, n_bt, msg);
    if (ca) return ca;
    std::vector<uint32_t> out;
    kmp_regex_groups_table t;
    std::string why;
    uint32_t ng = 0;
    for (uint32_t q = 0; q < n_rx; q++) {
        const uint32_t f = flags ? flags[q] : 0u, g = gate ? gate[q] : 0u;
        const int ce = check_expression(expr, flags, gate, q, n_pat, msg);
        if (ce) return ce;
        if (!(f & KMPGPU_RX_GROUPS)) continue;
        if (kmp_regex_compile_groups(expr[q], expr_len[q], f, &t, &why)) return refuse_pack(msg, "kmpgpu_set_regexes: expression %u: %s", q, why.c_str());
        const uint32_t qi = ng % KMP_RXG_TILE;
        if (qi == 0) out.resize(out.size() + KMP_RXG_TILE_WORDS, 0u);
        uint32_t *tile = out.data() + (size_t)(ng / KMP_RXG_TILE) * KMP_RXG_TILE_WORDS;
        const uint64_t sticky = t.eol ? 0ull : 1ull << t.n;
        for (uint32_t c = 0; c < 256u; c++) put64(tile + 2u * (c * KMP_RXG_TILE + qi), t.B[c] | sticky);
        uint32_t *rec = tile + 512u * KMP_RXG_TILE + 12u * qi;
        put64(rec, t.opt);
        put64(rec + 2, t.rep | sticky);
        put64(rec + 4, t.shift);
        put64(rec + 6, t.first);
        rec[8] = t.n | (t.bol ? 0u : 1u << 8) | ((f & KMPGPU_RX_GATED) ? 1u << 9 : 0u) | (t.eol ? 1u << 10 : 0u) | t.n_rules << 16;
        rec[9] = g;
        rec[10] = q;
        uint32_t *rules = tile + 512u * KMP_RXG_TILE + 12u * KMP_RXG_TILE + 4u * KMPGPU_RX_MAX_EDGES * qi;
        for (uint32_t r = 0; r < t.n_rules; r++) { put64(rules + 4u * r, t.src[r]); put64(rules + 4u * r + 2u, t.dst[r]); }
        ng++;
    }
    tables->swap(out);
    *n_groups = ng;
    return KMPGPU_OK;
}
