/* The parser of KMPGPU_FLOW_STREAMS's value (csrc/host/kmp_cli_streams.h) on its own, for AddressSanitizer + UBSan
 * (tests/test_streams_host.py): every string is handed over in a heap block of exactly its size, so a read behind its terminator is seen,
 * and the long digit strings would overflow an accumulator that did not stop at the maximum. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "kmp_cli_streams.h"

static int check(const char *s, int want_ok, uint32_t want_depth)
{
    char *copy = NULL;
    if (s) {
        copy = (char *)malloc(strlen(s) + 1);
        if (!copy) return 1;
        memcpy(copy, s, strlen(s) + 1);
    }
    uint32_t depth = 7777u;
    const int ok = kmp_cli_parse_depth(copy, &depth);
    free(copy);
    if (ok != want_ok || depth != (want_ok ? want_depth : 7777u)) {
        fprintf(stderr, "\"%s\": ok %d depth %u, wanted %d / %u\n", s ? s : "(null)", ok, depth, want_ok, want_depth);
        return 1;
    }
    return 0;
}

int main(void)
{
    int bad = 0;
    bad += check("1", 1, 1u);
    bad += check("98", 1, 98u);
    bad += check("0001", 1, 1u);
    bad += check("65536", 1, 65536u);
    bad += check("1073741824", 1, 1u << 30);
    bad += check("1k", 1, 1024u);
    bad += check("64k", 1, 65536u);
    bad += check("1048576k", 1, 1u << 30);
    bad += check("1m", 1, 1u << 20);
    bad += check("1024m", 1, 1u << 30);
    static const char *const refused[] = {NULL, "", "0", "00", "0k", "0m", "-1", "+1", " 1", "1 ", "1\n", "k", "m", "1K", "1M", "1g", "1kk", "1km", "1k ",
                                          "1.5", "1e3", "0x10", "1073741825", "1048577k", "1025m", "4294967296", "4294967297", "18446744073709551616",
                                          "18446744073709551617k", "99999999999999999999999999999999999999999999999999", "9999999999999999999999m", "depth"};
    for (size_t i = 0; i < sizeof refused / sizeof refused[0]; i++) bad += check(refused[i], 0, 0);
    if (bad) return 1;
    puts("streams driver ok");
    return 0;
}
