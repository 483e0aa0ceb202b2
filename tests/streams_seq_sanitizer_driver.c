/* The host code kmpgpu_load_streams_ordered adds, on its own, for AddressSanitizer + UBSan (tests/test_streams_seq_host.py):
 *   the parser of KMPGPU_FLOW_STREAMS_ORDER's value (csrc/host/kmp_cli_streams_order.h), every string in a heap block of exactly its size;
 *   kmp_extract_tcp_seq on a TCP and a UDP frame cut to every capture length, each in a heap block of exactly that many bytes, so a read
 *   behind the captured bytes is seen: it returns what the extractor returns and, for an accepted frame, the 32 bits at T + 4;
 *   with a path as argv[1] and "tcp" or "udp" as argv[2], kmp_arena_from_pcap_seq over that capture: "seq <n>" and one number per line. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "kmphost.h"
#include "kmp_cli_streams_order.h"

static int check_order(const char *s, int want_ok, int want)
{
    char *copy = NULL;
    if (s) {
        copy = (char *)malloc(strlen(s) + 1);
        if (!copy) return 1;
        memcpy(copy, s, strlen(s) + 1);
    }
    int order = 77;
    const int ok = kmp_cli_parse_streams_order(copy, &order);
    free(copy);
    if (ok != want_ok || order != (want_ok ? want : 77)) {
        fprintf(stderr, "\"%s\": ok %d order %d, wanted %d / %d\n", s ? s : "(null)", ok, order, want_ok, want);
        return 1;
    }
    return 0;
}

/* an Ethernet + IPv4 frame with the given header length (in 32-bit words) and protocol, 40 bytes behind the IP header: for TCP a 24-byte
 * header (data offset 6) and 16 bytes of payload */
static uint32_t make_frame(uint8_t *f, uint32_t ihl_words, uint8_t proto, uint32_t seq)
{
    const uint32_t T = 14u + 4u * ihl_words, n = T + 40u;
    for (uint32_t i = 0; i < n; i++) f[i] = (uint8_t)(0x40u + i);
    f[14] = (uint8_t)(0x40u | ihl_words);
    f[23] = proto;
    f[T + 4u] = (uint8_t)(seq >> 24); f[T + 5u] = (uint8_t)(seq >> 16); f[T + 6u] = (uint8_t)(seq >> 8); f[T + 7u] = (uint8_t)seq;
    f[T + 12u] = 0x60u;
    return n;
}

static int check_frames(void)
{
    int bad = 0;
    static const uint32_t seqs[] = {0u, 1u, 0x01020304u, 0x80000000u, 0xFFFFFFFFu};
    for (uint32_t ihl = 4; ihl <= 15; ihl++)
        for (int p = 0; p < 2; p++)
            for (size_t q = 0; q < sizeof seqs / sizeof seqs[0]; q++) {
                uint8_t full[14 + 60 + 40];
                const int proto = p ? KMP_PROTO_TCP : KMP_PROTO_UDP;
                const uint32_t n = make_frame(full, ihl, p ? 6u : 17u, seqs[q]);
                for (uint32_t cl = 0; cl <= n; cl++) {
                    uint8_t *f = (uint8_t *)malloc(cl ? cl : 1);
                    if (!f) return 1;
                    memcpy(f, full, cl);
                    uint32_t o = 0, l = 0, seq = 0xDEADBEEFu;
                    const int want = p ? kmp_extract_tcp(f, cl, &o, &l) : kmp_extract_udp(f, cl, &o, &l);
                    const int got = kmp_extract_tcp_seq(f, cl, proto, &seq);
                    if (got != want || seq != (want ? seqs[q] : 0xDEADBEEFu)) {
                        fprintf(stderr, "ihl %u proto %d caplen %u: %d seq %08x, wanted %d / %08x\n", ihl, proto, cl, got, seq, want, seqs[q]);
                        bad++;
                    }
                    free(f);
                }
            }
    return bad;
}

int main(int argc, char **argv)
{
    int bad = 0;
    bad += check_order("seq", 1, KMP_CLI_STREAMS_ORDER_SEQ);
    bad += check_order("capture", 1, KMP_CLI_STREAMS_ORDER_CAPTURE);
    static const char *const refused[] = {NULL, "", "s", "se", "seq ", " seq", "seqq", "Seq", "SEQ", "c", "captur", "capture ", "captured", "Capture",
                                          "sequence", "0", "1", "seq\n", "capture,seq", "tcp"};
    for (size_t i = 0; i < sizeof refused / sizeof refused[0]; i++) bad += check_order(refused[i], 0, 0);
    bad += check_frames();
    if (argc > 2) {
        kmp_arena a;
        kmp_pkt_meta *meta = NULL;
        uint32_t *seq = NULL;
        char err[KMP_PCAP_ERRBUF] = "";
        const int proto = strcmp(argv[2], "tcp") ? KMP_PROTO_UDP : KMP_PROTO_TCP;
        if (kmp_arena_from_pcap_seq(argv[1], proto, NULL, NULL, &a, err, &meta, &seq)) { fprintf(stderr, "%s\n", err); return 1; }
        printf("seq %llu\n", (unsigned long long)a.n_pkts);
        for (uint64_t k = 0; k < a.n_pkts; k++) printf("%u %u %u\n", seq[k], meta[k].proto, a.len[k]);
        free(meta); free(seq);
        kmp_arena_free(&a);
        /* without the metadata */
        if (kmp_arena_from_pcap_seq(argv[1], proto, NULL, NULL, &a, err, NULL, &seq)) { fprintf(stderr, "%s\n", err); return 1; }
        free(seq);
        kmp_arena_free(&a);
    }
    if (bad) return 1;
    puts("streams seq driver ok");
    return 0;
}
