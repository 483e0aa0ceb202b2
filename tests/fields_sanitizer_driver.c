/* The parser of KMPGPU_HTTP_FIELD's value (csrc/host/kmp_cli_fields.h) on its own, for AddressSanitizer + UBSan
 * (tests/test_fields_host.py): every string is handed over in a heap block of exactly its size, so a read behind its terminator is seen. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "kmp_cli_fields.h"

static int check(const char *s, int want_ok, int want_field)
{
    char *copy = NULL;
    if (s) {
        copy = (char *)malloc(strlen(s) + 1);
        if (!copy) return 1;
        memcpy(copy, s, strlen(s) + 1);
    }
    int field = -7;
    const int ok = kmp_cli_parse_field(copy, &field);
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
    bad += check("method", 1, KMP_CLI_FIELD_METHOD);
    bad += check("raw_uri", 1, KMP_CLI_FIELD_RAW_URI);
    bad += check("status", 1, KMP_CLI_FIELD_STATUS);
    bad += check("headers", 1, KMP_CLI_FIELD_HEADERS);
    bad += check("body", 1, KMP_CLI_FIELD_BODY);
    bad += check("uri", 1, KMP_CLI_FIELD_URI);
    static const char *const refused[] = {NULL, "", "m", "metho", "methods", "method ", " method", "Method", "URI", "raw", "raw_ur", "raw_uri2", "raw-uri",
                                          "header", "headers\n", "bod", "bodyy", "stat", "status_code", "uri,body", "1", "http_uri", "cookie", "\xff"};
    for (size_t i = 0; i < sizeof refused / sizeof refused[0]; i++) bad += check(refused[i], 0, 0);
    if (bad) return 1;
    puts("fields driver ok");
    return 0;
}
