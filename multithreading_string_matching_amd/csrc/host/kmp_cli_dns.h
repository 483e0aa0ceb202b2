/*
 * kmp_cli_dns.h -- the value of KMPGPU_DNS_FIELD as bin/serial and bin/openmp_data (kmp_cli.c) read it.  No dependencies: the parser
 * is also built on its own under the sanitizers (tests/dns_sanitizer_driver.c).
 */
#ifndef KMP_CLI_DNS_H
#define KMP_CLI_DNS_H

#include <string.h>

#define KMP_CLI_DNS_NONE  0
#define KMP_CLI_DNS_QNAME 1   /* KMPGPU_DNS_FIELD=qname: the value of KMPGPU_DNS_QNAME (kmpgpu.h) */

/* "qname" or "qname,tcp", exactly: 1, *field and *tcp (a 2-byte length stands in front of every message: KMPGPU_DNS_TCP_PREFIX);
 * anything else (a NULL or empty string too): 0, both untouched */
static inline int kmp_cli_parse_dns(const char *s, int *field, int *tcp)
{
    if (!s) return 0;
    if (strcmp(s, "qname") == 0) { *field = KMP_CLI_DNS_QNAME; *tcp = 0; return 1; }
    if (strcmp(s, "qname,tcp") == 0) { *field = KMP_CLI_DNS_QNAME; *tcp = 1; return 1; }
    return 0;
}

#endif
