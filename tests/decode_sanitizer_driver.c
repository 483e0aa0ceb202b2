/* The parser of KMPGPU_DECODE's value (csrc/host/kmp_cli_decode.h) on its own, for AddressSanitizer + UBSan (tests/test_decode_host.py):
 * every string is handed over in a heap block of exactly its size, so a read behind its terminator is seen. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "kmp_cli_decode.h"

static int check(const char *s, int want_ok, int want_mode)
{
    char *copy = NULL;
    if (s) {
        copy = (char *)malloc(strlen(s) + 1);
        if (!copy) return 1;
        memcpy(copy, s, strlen(s) + 1);
    }
    int mode = -7;
    const int ok = kmp_cli_parse_decode(copy, &mode);
    free(copy);
    if (ok != want_ok || mode != (want_ok ? want_mode : -7)) {
        fprintf(stderr, "\"%s\": ok %d mode %d, wanted %d / %d\n", s ? s : "(null)", ok, mode, want_ok, want_mode);
        return 1;
    }
    return 0;
}

int main(void)
{
    int bad = 0;
    bad += check("percent", 1, KMP_CLI_DECODE_PERCENT);
    bad += check("percent+plus", 1, KMP_CLI_DECODE_PLUS);
    static const char *const refused[] = {NULL, "", "p", "percen", "percent+", "percent+plu", "percent+pluss", "percent+plus ", " percent", "Percent",
                                          "PERCENT", "plus", "percent plus", "percent,plus", "1", "percent\n", "percent+plus+plus", "%"};
    for (size_t i = 0; i < sizeof refused / sizeof refused[0]; i++) bad += check(refused[i], 0, 0);
    if (bad) return 1;
    puts("decode driver ok");
    return 0;
}
