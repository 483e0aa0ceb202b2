/*
 * kmp_cli_streams_order.h -- the value of KMPGPU_FLOW_STREAMS_ORDER as bin/serial and bin/openmp_data (kmp_cli.c) read it.  No
 * dependencies: the parser is also built on its own under the sanitizers (tests/streams_seq_sanitizer_driver.c).
 */
#ifndef KMP_CLI_STREAMS_ORDER_H
#define KMP_CLI_STREAMS_ORDER_H

#define KMP_CLI_STREAMS_ORDER_CAPTURE 0        /* kmpgpu_load_streams: capture order */
#define KMP_CLI_STREAMS_ORDER_SEQ     1        /* kmpgpu_load_streams_ordered: TCP sequence numbers */

/* "capture" or "seq", exactly: 1 and *order; anything else (a NULL or empty string, another case, a blank): 0, *order untouched */
static inline int kmp_cli_parse_streams_order(const char *s, int *order)
{
    static const char capture[] = "capture", seq[] = "seq";
    if (!s) return 0;
    const char *w = (*s == 'c') ? capture : seq;
    int i = 0;
    for (; w[i]; i++)
        if (s[i] != w[i]) return 0;                             /* (s ends here at the latest: its 0 differs from w[i]) */
    if (s[i]) return 0;
    *order = (w == seq) ? KMP_CLI_STREAMS_ORDER_SEQ : KMP_CLI_STREAMS_ORDER_CAPTURE;
    return 1;
}

#endif
