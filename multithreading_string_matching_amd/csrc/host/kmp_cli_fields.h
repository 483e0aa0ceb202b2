/*
 * kmp_cli_fields.h -- the value of KMPGPU_HTTP_FIELD as bin/serial and bin/openmp_data (kmp_cli.c) read it.  No dependencies: the parser
 * is also built on its own under the sanitizers (tests/fields_sanitizer_driver.c).
 */
#ifndef KMP_CLI_FIELDS_H
#define KMP_CLI_FIELDS_H

#include <string.h>

/* the values of KMPGPU_FIELD_* (kmpgpu.h), and the URI percent-decoded, which is no field of the library's */
#define KMP_CLI_FIELD_NONE    0
#define KMP_CLI_FIELD_METHOD  1   /* KMPGPU_HTTP_FIELD=method */
#define KMP_CLI_FIELD_RAW_URI 2   /* =raw_uri */
#define KMP_CLI_FIELD_STATUS  3   /* =status */
#define KMP_CLI_FIELD_HEADERS 4   /* =headers */
#define KMP_CLI_FIELD_BODY    5   /* =body */
#define KMP_CLI_FIELD_URI     6   /* =uri: raw_uri, then kmpgpu_load_decoded */

/* one of the six names, exactly: 1 and *field; anything else (a NULL or empty string too): 0, *field untouched */
static inline int kmp_cli_parse_field(const char *s, int *field)
{
    static const char *const names[] = {"method", "raw_uri", "status", "headers", "body", "uri"};
    if (!s) return 0;
    for (int i = 0; i < 6; i++)
        if (strcmp(s, names[i]) == 0) { *field = KMP_CLI_FIELD_METHOD + i; return 1; }
    return 0;
}

#endif
