/*
 * kmp_regex.h -- the expressions of kmpgpu_set_regexes (kmpgpu.h) compiled into position automata, and the host interpreter that states
 * the algorithm the kernel of kmp_regex.hip runs.  Host code without a HIP header, as kmp_tables.h: it builds and runs without a device
 * (tests/regex_sanitizer_driver.cpp).
 *
 * An expression is a sequence of at most KMPGPU_RX_MAX_POSITIONS positions, each a byte class that is mandatory or optional and taken once
 * or repeatedly: C{n,m} is n mandatory positions and m - n optional ones, C{n,} n - 1 mandatory ones and a mandatory repeatable one, C* one
 * optional repeatable position, C+ one repeatable one.  A text is matched with a reach set R of n + 1 bits -- bit i: position i is next,
 * bit n: accepted -- stepped once per byte (kmp_regex_search).
 */
#ifndef KMP_REGEX_H
#define KMP_REGEX_H

#include <stddef.h>
#include <stdint.h>

#include <string>

#include "kmpgpu.h"

/* The kernel takes the expressions KMP_RX_TILE at a time out of LDS (kmp_regex.hip).  One tile of the device table, as kmp_pack_regexes lays it
 * out: B[256][KMP_RX_TILE] as 64-bit words -- the tile's words of one byte side by side, what a lane reads per text byte -- then
 * KMP_RX_TILE records of 32 bytes: {opt, rep as 64-bit words, n | restart << 8 | gated << 9 | eol << 10 | opt_run << 16, gate, 0, 0}; restart:
 * no leading ^.  In the device table an expression without $ has bit n set in every B word and in rep: once accepted it stays accepted.
 * The slots behind the last expression of the last tile are zero. */
#define KMP_RX_TILE 8u
#define KMP_RX_TILE_WORDS (512u * KMP_RX_TILE + 8u * KMP_RX_TILE)     /* uint32_t per tile */

struct kmp_regex_table {
    uint64_t B[256];        /* bit p of B[c]: byte c is in the class of position p.  KMPGPU_RX_NOCASE and KMPGPU_RX_DOTALL live here alone */
    uint64_t opt, rep;      /* the optional positions, the repeatable ones */
    uint32_t n;             /* positions, 1 .. KMPGPU_RX_MAX_POSITIONS */
    uint32_t opt_run;       /* the longest run of consecutive optional positions: the steps closure() needs at most */
    bool     bol, eol;      /* a leading ^, a trailing $ */
};

/* KMPGPU_OK with *table, or KMPGPU_EINVAL with "position P: what is wrong there" in *msg (P: a byte index of expr) and *table undefined.
 * flags: KMPGPU_RX_NOCASE | KMPGPU_RX_DOTALL; every other bit is the caller's (kmp_pack_regexes checks them). */
int kmp_regex_compile(const uint8_t *expr, size_t len, uint32_t flags, kmp_regex_table *table, std::string *msg);

/* Are there 0 <= s <= e <= E with text[s:e] in the expression's language, s == 0 under ^, e == E under $?  Reads text[0 .. E - 1]. */
bool kmp_regex_search(const kmp_regex_table &table, const uint8_t *text, size_t E);

/* ---- expressions under KMPGPU_RX_GROUPS: groups and alternation (kmp_regex_groups.hip) ----
 *
 * The expression is unrolled -- G{n,m}: n copies of G and m - n optional ones, G{n,}: n - 1 copies and one G+, G*: an optional G+ -- and
 * its positions are numbered left to right.  Its Glushkov sets: FIRST (plus bit n where the expression matches the empty string) and,
 * per position j, F(j) = follow(j) (plus bit n where j may be last).  The reach set R keeps its meaning -- bit i: position i may take the
 * next byte, bit n: accepted -- and one step on byte c is
 *     b = R & B[c];  N = (b & SHIFT) << 1 | b & REP | OR over the rules r with (b & src[r]) != 0 of dst[r];  R = closure(N) | (no ^ ? FIRST : 0)
 * with closure() the carry-add of kmp_regex.hip over OPT.  The sets are functions of F alone:
 *     SHIFT = { j : j + 1 in F(j) }     REP = { j : j in F(j) }
 *     OPT   = { i : i in F(j) => i + 1 in F(j) for every j, and i in FIRST => i + 1 in FIRST }
 * and so are the rules: T(j) is what of F(j) closure(shift and repeat part of j) does not give and whose left neighbour is not both in F(j)
 * and in OPT; the positions with the same non-empty T are one rule {src, dst = T}.  The compiler checks closure(shift_j | rep_j | T(j)) ==
 * F(j) for every j and closure(FIRST) == FIRST.  An expression without ( ) | has no rule and steps as kmp_regex_search does.
 *
 * The kernel takes them KMP_RXG_TILE at a time.  One tile of the device table, as kmp_pack_regex_groups lays it out:
 * B[256][KMP_RXG_TILE] as 64-bit words, then KMP_RXG_TILE records of 48 bytes: {opt, rep, shift, first as 64-bit words,
 * n | restart << 8 | gated << 9 | eol << 10 | n_rules << 16, gate, q, 0} -- q: the expression's index, whose row of the matrix it writes --
 * then KMP_RXG_TILE x KMPGPU_RX_MAX_EDGES rules of 16 bytes {src, dst}, the unused ones zero.  Bit n is sticky as in the linear table. */
#define KMP_RXG_TILE 4u
#define KMP_RXG_TILE_WORDS (512u * KMP_RXG_TILE + 12u * KMP_RXG_TILE + 4u * KMPGPU_RX_MAX_EDGES * KMP_RXG_TILE)     /* uint32_t per tile */
#define KMP_RXG_MAX_DEPTH 32     /* groups nest this deep at most */

struct kmp_regex_groups_table {
    uint64_t B[256];
    uint64_t opt, rep, shift, first;    /* first: FIRST, with bit n where the expression matches the empty string */
    uint64_t src[KMPGPU_RX_MAX_EDGES], dst[KMPGPU_RX_MAX_EDGES];
    uint32_t n, n_rules;
    bool     bol, eol;
};

/* As kmp_regex_compile, in the dialect of KMPGPU_RX_GROUPS (kmpgpu.h). */
int kmp_regex_compile_groups(const uint8_t *expr, size_t len, uint32_t flags, kmp_regex_groups_table *table, std::string *msg);

/* As kmp_regex_search: the host statement of what kmp_regex_groups_kernel runs. */
bool kmp_regex_search_groups(const kmp_regex_groups_table &table, const uint8_t *text, size_t E);

#endif
