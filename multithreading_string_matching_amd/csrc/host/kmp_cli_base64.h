/*
 * kmp_cli_base64.h -- the value of KMPGPU_BASE64 as bin/serial and bin/openmp_data (kmp_cli.c) read it.  No dependencies: the parser is
 * also built on its own under the sanitizers (tests/base64_sanitizer_driver.c).
 */
#ifndef KMP_CLI_BASE64_H
#define KMP_CLI_BASE64_H

#include <string.h>

#define KMP_CLI_BASE64_MIN_RUN_LO 4u
#define KMP_CLI_BASE64_MIN_RUN_HI 255u    /* the range of kmpgpu_load_base64's min_run */

/* "<min_run>" or "<min_run>,url", exactly: decimal digits without sign or blanks that come to 4..255, then nothing or ",url": 1, and
 * *min_run and *urlsafe; anything else (a NULL or empty string too): 0, both untouched */
static inline int kmp_cli_parse_base64(const char *s, unsigned *min_run, int *urlsafe)
{
    if (!s) return 0;
    unsigned v = 0;
    size_t i = 0;
    while (s[i] >= '0' && s[i] <= '9') {
        v = v * 10u + (unsigned)(s[i] - '0');
        if (v > KMP_CLI_BASE64_MIN_RUN_HI) return 0;        /* (also: no overflow, however long the digits go on) */
        i++;
    }
    if (i == 0 || v < KMP_CLI_BASE64_MIN_RUN_LO) return 0;
    int url = 0;
    if (s[i]) {
        if (strcmp(s + i, ",url") != 0) return 0;
        url = 1;
    }
    *min_run = v;
    *urlsafe = url;
    return 1;
}

#endif
