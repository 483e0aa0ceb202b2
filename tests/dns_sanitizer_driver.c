/* The parser of KMPGPU_DNS_FIELD's value (csrc/host/kmp_cli_dns.h) on its own, for AddressSanitizer + UBSan
 * (tests/test_dns_host.py): every string is handed over in a heap block of exactly its size, so a read behind its terminator is seen. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "kmp_cli_dns.h"

static int check(const char *s, int want_ok, int want_field, int want_tcp)
{
    char *copy = NULL;
    if (s) {
        copy = (char *)malloc(strlen(s) + 1);
        if (!copy) return 1;
        memcpy(copy, s, strlen(s) + 1);
    }
    int field = -7, tcp = -9;
    const int ok = kmp_cli_parse_dns(copy, &field, &tcp);
    free(copy);
    if (ok != want_ok || field != (want_ok ? want_field : -7) || tcp != (want_ok ? want_tcp : -9)) {
        fprintf(stderr, "\"%s\": ok %d field %d tcp %d, wanted %d / %d / %d\n", s ? s : "(null)", ok, field, tcp, want_ok, want_field, want_tcp);
        return 1;
    }
    return 0;
}

int main(void)
{
    int bad = 0;
    bad += check("qname", 1, KMP_CLI_DNS_QNAME, 0);
    bad += check("qname,tcp", 1, KMP_CLI_DNS_QNAME, 1);
    static const char *const refused[] = {NULL, "", "q", "qnam", "qnames", "qname ", " qname", "QNAME", "Qname", "qname,", "qname,t", "qname,tc", "qname,tcp ",
                                          "qname,tcp,", "qname,tcp,tcp", "qname,TCP", "qname,udp", "qname;tcp", "qname tcp", ",tcp", "tcp", "tcp,qname",
                                          "qname\n", "name", "dns.query", "dns_query", "1", "\xff"};
    for (size_t i = 0; i < sizeof refused / sizeof refused[0]; i++) bad += check(refused[i], 0, 0, 0);
    if (bad) return 1;
    puts("dns driver ok");
    return 0;
}
