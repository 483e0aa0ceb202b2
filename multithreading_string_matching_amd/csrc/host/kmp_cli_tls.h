/*
 * kmp_cli_tls.h -- the value of KMPGPU_TLS_FIELD as bin/serial and bin/openmp_data (kmp_cli.c) read it.  No dependencies: the parser
 * is also built on its own under the sanitizers (tests/tls_sanitizer_driver.c).
 */
#ifndef KMP_CLI_TLS_H
#define KMP_CLI_TLS_H

#include <string.h>

#define KMP_CLI_TLS_NONE 0
#define KMP_CLI_TLS_SNI  1   /* KMPGPU_TLS_FIELD=sni: the value of KMPGPU_TLS_SNI (kmpgpu.h) */
#define KMP_CLI_TLS_ALPN 2   /* KMPGPU_TLS_FIELD=alpn: the value of KMPGPU_TLS_ALPN */

/* "sni" or "alpn", exactly: 1 and *field; anything else (a NULL or empty string too): 0, *field untouched */
static inline int kmp_cli_parse_tls(const char *s, int *field)
{
    if (!s) return 0;
    if (strcmp(s, "sni") == 0) { *field = KMP_CLI_TLS_SNI; return 1; }
    if (strcmp(s, "alpn") == 0) { *field = KMP_CLI_TLS_ALPN; return 1; }
    return 0;
}

#endif
