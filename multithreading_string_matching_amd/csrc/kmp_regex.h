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

#endif
