/*
 * kmp_cli_decode.h -- the value of KMPGPU_DECODE as bin/serial and bin/openmp_data (kmp_cli.c) read it.  No dependencies: the parser is
 * also built on its own under the sanitizers (tests/decode_sanitizer_driver.c).
 */
#ifndef KMP_CLI_DECODE_H
#define KMP_CLI_DECODE_H

#include <string.h>

#define KMP_CLI_DECODE_NONE    0
#define KMP_CLI_DECODE_PERCENT 1   /* KMPGPU_DECODE=percent */
#define KMP_CLI_DECODE_PLUS    2   /* KMPGPU_DECODE=percent+plus: a '+' decodes to a space as well */

/* "percent" or "percent+plus", exactly: 1 and *mode; anything else (a NULL or empty string too): 0, *mode untouched */
static inline int kmp_cli_parse_decode(const char *s, int *mode)
{
    if (!s) return 0;
    if (strcmp(s, "percent") == 0) { *mode = KMP_CLI_DECODE_PERCENT; return 1; }
    if (strcmp(s, "percent+plus") == 0) { *mode = KMP_CLI_DECODE_PLUS; return 1; }
    return 0;
}

#endif
