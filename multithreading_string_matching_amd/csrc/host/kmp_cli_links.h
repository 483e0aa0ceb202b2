/* kmp_cli_links.h -- the buffer word of a line of KMPGPU_LINKS_FILE, <kind>:<value>, where <value> is what the variable of that buffer
 * takes and is parsed by that variable's own parser:
 *     http:method|raw_uri|uri|status|headers|body      (KMPGPU_HTTP_FIELD, kmp_cli_fields.h)
 *     dns:qname[,tcp]                                  (KMPGPU_DNS_FIELD, kmp_cli_dns.h)
 *     decode:percent[+plus]                            (KMPGPU_DECODE, kmp_cli_decode.h)
 *     base64:<min_run>[,url]                           (KMPGPU_BASE64, kmp_cli_base64.h)
 * Host code without a GPU call, so that tests/links_sanitizer_driver.cpp drives it as it is. */
#ifndef KMP_CLI_LINKS_H
#define KMP_CLI_LINKS_H

#include <string.h>

#include "kmp_cli_base64.h"
#include "kmp_cli_decode.h"
#include "kmp_cli_dns.h"
#include "kmp_cli_fields.h"

#define KMP_CLI_LINK_HTTP   1
#define KMP_CLI_LINK_DNS    2
#define KMP_CLI_LINK_DECODE 3
#define KMP_CLI_LINK_BASE64 4
#define KMP_CLI_LINK_BUFFERS_MAX 8       /* distinct buffers of one links file: a context per buffer and shard */

typedef struct kmp_cli_link_buffer {
    int kind;                             /* KMP_CLI_LINK_* */
    int field;                            /* http: KMP_CLI_FIELD_*; dns: KMP_CLI_DNS_*; decode: KMP_CLI_DECODE_* */
    int flag;                             /* dns: ",tcp"; base64: ",url" */
    unsigned min_run;                     /* base64 */
} kmp_cli_link_buffer;

/* 1 and *out, or 0 for a word that names no buffer */
static inline int kmp_cli_parse_link_buffer(const char *s, kmp_cli_link_buffer *out)
{
    if (!s) return 0;
    memset(out, 0, sizeof *out);
    if (strncmp(s, "http:", 5) == 0) { out->kind = KMP_CLI_LINK_HTTP; return kmp_cli_parse_field(s + 5, &out->field); }
    if (strncmp(s, "dns:", 4) == 0) { out->kind = KMP_CLI_LINK_DNS; return kmp_cli_parse_dns(s + 4, &out->field, &out->flag); }
    if (strncmp(s, "decode:", 7) == 0) { out->kind = KMP_CLI_LINK_DECODE; return kmp_cli_parse_decode(s + 7, &out->field); }
    if (strncmp(s, "base64:", 7) == 0) { out->kind = KMP_CLI_LINK_BASE64; return kmp_cli_parse_base64(s + 7, &out->min_run, &out->flag); }
    return 0;
}

/* two words that name the same buffer (the same kind and value, however they were spelt) */
static inline int kmp_cli_link_buffer_same(const kmp_cli_link_buffer *a, const kmp_cli_link_buffer *b)
{
    return a->kind == b->kind && a->field == b->field && a->flag == b->flag && a->min_run == b->min_run;
}

#endif
