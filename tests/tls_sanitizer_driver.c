/* The parser of KMPGPU_TLS_FIELD's value (csrc/host/kmp_cli_tls.h) on its own, for AddressSanitizer + UBSan
 * (tests/test_tls_host.py): every string is handed over in a heap block of exactly its size, so a read behind its terminator is seen. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "kmp_cli_tls.h"

static int check(const char *s, int want_ok, int want_field)
{
    char *copy = NULL;
    if (s) {
        copy = (char *)malloc(strlen(s) + 1);
        if (!copy) return 1;
        memcpy(copy, s, strlen(s) + 1);
    }
    int field = -7;
    const int ok = kmp_cli_parse_tls(copy, &field);
    free(copy);
    if (ok != want_ok || field != (want_ok ? want_field : -7)) {
        fprintf(stderr, "\"%s\": ok %d field %d, wanted %d / %d\n", s ? s : "(null)", ok, field, want_ok, want_field);
        return 1;
    }
    return 0;
}

int main(void)
{
    int bad = 0;
    bad += check("sni", 1, KMP_CLI_TLS_SNI);
    bad += check("alpn", 1, KMP_CLI_TLS_ALPN);
    static const char *const refused[] = {NULL, "", "s", "sn", "snis", "sni ", " sni", "SNI", "Sni", "sni,", "sni,alpn", "alpn,sni", "alp", "alpns", "alpn ",
                                          "ALPN", "alpn,", "sni\n", "alpn\n", "tls.sni", "tls_sni", "server_name", "host", "ja3", "1", "2", "\xff"};
    for (size_t i = 0; i < sizeof refused / sizeof refused[0]; i++) bad += check(refused[i], 0, 0);
    if (KMP_CLI_TLS_NONE != 0 || KMP_CLI_TLS_SNI != 1 || KMP_CLI_TLS_ALPN != 2) bad++;
    if (bad) return 1;
    puts("tls driver ok");
    return 0;
}
