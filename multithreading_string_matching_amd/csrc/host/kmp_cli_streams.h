/*
 * kmp_cli_streams.h -- the value of KMPGPU_FLOW_STREAMS as bin/serial and bin/openmp_data (kmp_cli.c) read it.  No dependencies: the parser
 * is also built on its own under the sanitizers (tests/streams_sanitizer_driver.c).
 */
#ifndef KMP_CLI_STREAMS_H
#define KMP_CLI_STREAMS_H

#include <stdint.h>

#define KMP_CLI_STREAM_DEPTH_MAX (1u << 30)        /* KMPGPU_STREAM_DEPTH_MAX */

/* A depth: decimal digits, nothing in front of them, with an optional k (x 1024) or m (x 1048576) behind them, 1 .. 2^30 in all: 1 and
 * *depth; anything else (a NULL or empty string, a sign, a blank, a value out of range): 0, *depth untouched */
static inline int kmp_cli_parse_depth(const char *s, uint32_t *depth)
{
    uint64_t v = 0;
    if (!s || *s < '0' || *s > '9') return 0;
    for (; *s >= '0' && *s <= '9'; s++) {
        v = v * 10u + (uint64_t)(*s - '0');
        if (v > KMP_CLI_STREAM_DEPTH_MAX) return 0;             /* (before the next digit can overflow) */
    }
    if (*s == 'k' || *s == 'm') v <<= (*s++ == 'k') ? 10 : 20;
    if (*s || v < 1u || v > KMP_CLI_STREAM_DEPTH_MAX) return 0;
    *depth = (uint32_t)v;
    return 1;
}

#endif
