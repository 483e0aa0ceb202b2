/* The parser of KMPGPU_BASE64's value (csrc/host/kmp_cli_base64.h) on its own, for AddressSanitizer + UBSan (tests/test_base64_host.py):
 * every string is handed over in a heap block of exactly its size, so a read behind its terminator is seen. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "kmp_cli_base64.h"

static int check(const char *s, int want_ok, unsigned want_run, int want_url)
{
    char *copy = NULL;
    if (s) {
        copy = (char *)malloc(strlen(s) + 1);
        if (!copy) return 1;
        memcpy(copy, s, strlen(s) + 1);
    }
    unsigned run = 7777u;
    int url = -7;
    const int ok = kmp_cli_parse_base64(copy, &run, &url);
    free(copy);
    if (ok != want_ok || run != (want_ok ? want_run : 7777u) || url != (want_ok ? want_url : -7)) {
        fprintf(stderr, "\"%s\": ok %d run %u url %d, wanted %d / %u / %d\n", s ? s : "(null)", ok, run, url, want_ok, want_run, want_url);
        return 1;
    }
    return 0;
}

int main(void)
{
    int bad = 0;
    bad += check("4", 1, 4u, 0);
    bad += check("16", 1, 16u, 0);
    bad += check("255", 1, 255u, 0);
    bad += check("4,url", 1, 4u, 1);
    bad += check("24,url", 1, 24u, 1);
    bad += check("255,url", 1, 255u, 1);
    bad += check("016", 1, 16u, 0);
    static const char *const refused[] = {NULL, "", "3", "0", "256", "1000", "4294967300", "99999999999999999999999999", "-16", "+16", " 16", "16 ",
                                          "16,", "16,ur", "16,url ", "16,urls", "16,URL", "16;url", "16 url", ",url", "url", "0x10", "1e2", "16\n",
                                          "16,url,url", "3,url", "256,url", "sixteen", "1 6"};
    for (size_t i = 0; i < sizeof refused / sizeof refused[0]; i++) bad += check(refused[i], 0, 0u, 0);
    if (bad) return 1;
    puts("base64 driver ok");
    return 0;
}
