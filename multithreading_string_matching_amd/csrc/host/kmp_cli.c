/*
 * kmp_cli.c -- the reference's command lines on top of the MI355X hot path.
 *
 * Built twice (csrc/Makefile):
 *   bin/serial       ./serial <file.pcap> <string.txt> [udp/tcp]                     serial.c:2-3,33-51
 *   bin/openmp_data  ./openmp_data <file.pcap> <string.txt> thread_number [tcp/udp]  openmp_data.c:1-2,35-54
 * In the second form thread_number is the number of GPU shards: the payloads are split into
 * contiguous ranges the way mpi_dumping.c:149-157 splits them over ranks (N/P each, remainder to
 * shard 0) and the per-shard counts are summed (mpi_dumping.c:202).
 *
 * stdout is byte-compatible with the reference (serial.c:163-169); throughput details go to
 * stderr.  There is no CPU fallback: without a gfx950 device the program fails with exit code 2.
 *
 * KMPGPU_DEVICE_EXTRACT=1: the raw capture is uploaded and the payload extraction
 * (openmp_data.c:128-147, packet_dumping.h:87-188) runs on the GPU (kmpgpu_load_frames).
 *
 * Extension (the reference prints counts only, serial.c:163-166): with the environment variable
 * KMPGPU_OFFSETS_FILE=<path> every match is also written to <path> as "payload,offset,pattern"
 * lines (payload = index among the extracted payloads, pattern = index in the pattern file).
 * KMPGPU_PACKETS_FILE=<path>: which payloads hold which patterns (kmpgpu_scan_alerts over the rows of kmpgpu_scan_packets), one "payload,pattern" line per
 * pair that holds at least one match, sorted by payload, then by pattern (indices as in the offsets file).
 *
 * KMPGPU_RULES_FILE=<rules> with KMPGPU_ALERTS_FILE=<path>: content rules over the patterns (kmpgpu_set_rules, kmpgpu_scan_alerts; the
 * file format is kmp_rules_parse's, kmphost.h: one rule per line, terms are indices into the pattern file, "!" in front of one that
 * must not be in the payload), one "payload,rule" line per payload that a rule matches, sorted by payload, then by rule (rule =
 * index among the rule lines).  One of the two without the other, or a rules file that does not parse: message on stderr, exit 1,
 * before any GPU work.  Both go together with KMPGPU_NOCASE, KMPGPU_WHOLE_PAYLOAD, KMPGPU_DEVICE_EXTRACT and KMPGPU_PACKETS_FILE.
 *
 * KMPGPU_RELATIONS_FILE=<relations>, together with KMPGPU_RULES_FILE and KMPGPU_ALERTS_FILE: distance / within relations between two
 * patterns (kmpgpu_set_relations; the file format is kmp_relations_parse's, kmphost.h: "<a> <b> <dmin> <dmax>" per line, '*' for an
 * unbounded side), set on every shard's context before the rules, whose file may then name relation q as "r<q>" / "!r<q>"
 * (kmp_rules_parse_rel).  A relations file that does not parse, or the variable without the other two: message on stderr, exit 1,
 * before any GPU work.  stdout is what it is without the variable.
 *
 * KMPGPU_CHAINS_FILE=<chains>, together with KMPGPU_RULES_FILE and KMPGPU_ALERTS_FILE, with or without KMPGPU_RELATIONS_FILE: content
 * chains, each content relative to the match before it (kmpgpu_set_chains; the file format is kmp_chains_parse's, kmphost.h:
 * "<p0> <dmin> <dmax> <p1> [<dmin> <dmax> <p2> ...]" per line), set on every shard's context behind the relations and before the rules,
 * whose file may then name chain q as "c<q>" / "!c<q>" (kmp_rules_parse_terms).  A chains file that does not parse, or the variable
 * without the other two: message on stderr, exit 1, before any GPU work.  stdout is what it is without the variable.
 *
 * KMPGPU_HEADERS_FILE=<headers>, together with KMPGPU_RULES_FILE and KMPGPU_ALERTS_FILE, with or without the relations and chains files:
 * header predicates on addresses, ports, protocol and payload length (kmpgpu_set_headers; the file format is kmp_headers_parse's, kmphost.h:
 * "<proto> <src> <sport> <dir> <dst> <dport> [<len>]" per line), set on every shard's context behind the chains and before the rules, whose
 * file may then name predicate q as "h<q>" / "!h<q>" (kmp_rules_parse_hdr).  The payloads' header fields come from the host extraction
 * (kmp_arena_from_pcap_meta, kmpgpu_set_meta of the shard's slice) or, with KMPGPU_DEVICE_EXTRACT=1, from the device's
 * (KMPGPU_OPT_KEEP_META); both routes write the same files.  A headers file that does not parse, or the variable without the other two:
 * message on stderr, exit 1, before any GPU work.  stdout is what it is without the variable.
 *
 * KMPGPU_BYTETESTS_FILE=<byte tests>, together with KMPGPU_RULES_FILE and KMPGPU_ALERTS_FILE and / or KMPGPU_FLOW_ALERTS_FILE, with or without
 * the relations, chains and headers files: numeric fields of the payload as rule terms (kmpgpu_set_bytetests; the file format is
 * kmp_bytetests_parse's, kmphost.h: "<nbytes> <op> <value> <offset> [after <pattern index>] [little] [mask <m>]" per line), set on every
 * shard's context behind the header predicates and before the rules, whose file may then name test q as "b<q>" / "!b<q>"
 * (kmp_rules_parse_bt).  A byte tests file that does not parse, or the variable without the rules and an alerts file: message on stderr,
 * exit 1, before any GPU work.  stdout is what it is without the variable.
 *
 * KMPGPU_REGEX_FILE=<expressions>, together with KMPGPU_RULES_FILE and KMPGPU_ALERTS_FILE and / or KMPGPU_FLOW_ALERTS_FILE, with or without the
 * relations, chains, headers and byte tests files: expressions of byte classes and repeats as rule terms (kmpgpu_set_regexes; the file format
 * is kmp_regexes_parse's, kmphost.h: "/EXPR/[i][s] [with <pattern index>]" per line, the dialect kmpgpu.h's), set on every shard's context
 * behind the byte tests and before the rules, whose file may then name expression q as "x<q>" / "!x<q>" (kmp_rules_parse_rx).  An
 * expressions file that does not parse, or the variable without the rules and an alerts file: message on stderr, exit 1, before any GPU
 * work; an expression outside the dialect is refused by kmpgpu_set_regexes when the shard is set up.  stdout is what it is without the
 * variable.
 *
 * KMPGPU_WINDOWS_FILE=<windows>: per-pattern offset windows (kmpgpu_set_windows; the file format is kmp_windows_parse's, kmphost.h:
 * "<pattern index> <first> <last>" per line, '*' for no upper bound) on every shard's context.  They take effect on the files written
 * for KMPGPU_OFFSETS_FILE, KMPGPU_PACKETS_FILE and KMPGPU_RULES_FILE + KMPGPU_ALERTS_FILE: only the matches that start inside their
 * pattern's window are listed, mark a payload or feed a rule.  stdout -- the counts -- is what it is without windows.  A windows
 * file that does not parse, or one set without any of those output files (it has no effect): message on stderr, exit 1, before
 * any GPU work.
 *
 * KMPGPU_EXPORT_FILE=<out.pcap>: the payloads that hold at least one pattern (any of kmpgpu_scan_packets) -- with KMPGPU_RULES_FILE set,
 * the payloads that at least one rule matches (any of kmpgpu_scan_rules) -- written as a capture, in payload order over all shards.
 * Per shard the selection is compacted on the device into a second context (kmpgpu_load_selected) and only the selected bytes are
 * downloaded.  The frames are the synthetic Ethernet/IPv4/UDP frames of kmp_write_udp_pcap around the payloads, also in tcp mode: the
 * capture's own headers are not kept.  Windows (KMPGPU_WINDOWS_FILE) decide what a hit is here as in the packets file; with
 * KMPGPU_RULES_FILE, KMPGPU_ALERTS_FILE may be left out when this variable is set.  A path that cannot be written: message on stderr,
 * exit 1, before any GPU work.  stdout is what it is without the variable.
 *
 * KMPGPU_FLOWS_FILE=<path>: the payloads grouped by the 5-tuple of their header fields on the device (kmpgpu_flows_build), one line per flow,
 * "flow,proto,src,sport,dst,dport,first_payload,last_payload,payloads,bytes": flows are numbered in the order of their first payload,
 * the addresses are dotted quads and, with the ports, those of the flow's first payload.  KMPGPU_FLOWS_DIRECTED=1: the two directions of
 * a conversation are two flows.  KMPGPU_FLOW_ALERTS_FILE=<path>, together with KMPGPU_RULES_FILE (KMPGPU_ALERTS_FILE may be left out):
 * the rules evaluated per flow (kmpgpu_scan_flows, KMPGPU_FLOW_SCOPE_FLOW: a rule's contents may lie in different payloads of the
 * connection), one "flow,rule" line per flow a rule matches, sorted by flow, then by rule.  The header fields come the way they do for
 * KMPGPU_HEADERS_FILE, and both routes write the same files.  Refused with a message on stderr and exit 1, before any GPU work: more
 * than one shard (a flow would be cut at a shard's edge), KMPGPU_FLOW_ALERTS_FILE without a rules file, a path that cannot be written.
 * stdout is what it is without the variables.
 *
 * KMPGPU_FLOW_SEAMS=<reach>, together with KMPGPU_FLOW_ALERTS_FILE: contents split across two consecutive payloads of a flow direction
 * count as present in the flow.  A second context on the shard's device gets the seams of the capture (kmpgpu_load_seams: per payload
 * with a predecessor in its flow and direction, the predecessor's last <reach> bytes and the payload's first <reach> bytes) and the same
 * patterns under the same text rule and case rule, and the flow alerts come from kmpgpu_scan_flows_seams.  The windows of
 * KMPGPU_WINDOWS_FILE count from a payload's start and stay with the payloads: the seams are scanned without windows.  Refused with a
 * message on stderr and exit 1, before any GPU work: the variable without KMPGPU_FLOW_ALERTS_FILE, a reach that is no number in 1..98.
 *
 * KMPGPU_DECODE=percent or KMPGPU_DECODE=percent+plus, together with at least one of KMPGPU_PACKETS_FILE, KMPGPU_ALERTS_FILE and
 * KMPGPU_FLOW_ALERTS_FILE: these row outputs are decided on the percent-decoded payloads (kmpgpu_load_decoded; with +plus a '+' decodes
 * to a space as well), so that `GET /%61dmin` meets the rule that names `/admin`.  Per shard a second context on the shard's device gets
 * the decoding of the shard's arena, every payload, so the payload numbers are the capture's, and the same patterns and flags, windows,
 * relations, chains, header predicates, byte tests, expressions, rules and text rule as the shard's (upload_tables).  stdout -- the
 * counts over the payloads as captured -- and KMPGPU_FLOWS_FILE are what they are without the variable.  Refused with a message on
 * stderr and exit 1, before any GPU work: any other value; the variable together with KMPGPU_OFFSETS_FILE (offsets in decoded payloads
 * are not mapped back), KMPGPU_EXPORT_FILE or KMPGPU_FLOW_SEAMS; the variable with none of the three row outputs.
 *
 * KMPGPU_HTTP_FIELD=method|raw_uri|uri|status|headers|body, together with at least one of KMPGPU_PACKETS_FILE, KMPGPU_ALERTS_FILE and
 * KMPGPU_FLOW_ALERTS_FILE: these row outputs are decided on that field of the HTTP message at the start of every payload
 * (kmpgpu_load_fields; the definition: kmpgpu.h), so that a rule that names `/admin` meets the request line and not a Referer: header or a
 * body.  Per shard a second context on the shard's device gets the same tables as the shard's (upload_tables) and the field buffer of the
 * shard's arena, every payload (an absent field is an empty payload), so the payload numbers are the capture's; `uri` is raw_uri
 * percent-decoded (kmpgpu_load_decoded) through a third context.  stdout and KMPGPU_FLOWS_FILE are what they are without the variable.
 * Refused with a message on stderr and exit 1, before any GPU work: any other value; the variable together with KMPGPU_DECODE,
 * KMPGPU_OFFSETS_FILE, KMPGPU_EXPORT_FILE, KMPGPU_FLOW_SEAMS, KMPGPU_FLOW_STREAMS, KMPGPU_FLOWBITS_FILE or KMPGPU_THRESHOLDS_FILE; the
 * variable with none of the three row outputs.
 *
 * KMPGPU_BASE64=<min_run>[,url], together with at least one of KMPGPU_PACKETS_FILE, KMPGPU_ALERTS_FILE and KMPGPU_FLOW_ALERTS_FILE: these
 * row outputs are decided on the payloads with their base64 runs of <min_run> (4..255) alphabet bytes and more decoded
 * (kmpgpu_load_base64; the definition: kmpgpu.h; ,url: the alphabet that ends in - _), so that `Authorization: Basic YWRtaW46YWRtaW4=`
 * meets the rule that names `admin:admin`.  Per shard a second context on the shard's device gets the same tables as the shard's
 * (upload_tables) and the decoding of the shard's arena, every payload, so the payload numbers are the capture's.  stdout and
 * KMPGPU_FLOWS_FILE are what they are without the variable.  Refused with a message on stderr and exit 1, before any GPU work: any other
 * value; the variable together with KMPGPU_DECODE, KMPGPU_HTTP_FIELD, KMPGPU_OFFSETS_FILE, KMPGPU_EXPORT_FILE, KMPGPU_FLOW_SEAMS,
 * KMPGPU_FLOW_STREAMS, KMPGPU_FLOWBITS_FILE or KMPGPU_THRESHOLDS_FILE; the variable with none of the three row outputs.
 *
 * KMPGPU_LINKS_FILE=<links>, together with KMPGPU_RULES_FILE: one rule over several buffers of the same payloads.  One link per line,
 * "<buffer> <term>" (kmp_links_parse, kmphost.h; the buffer words: kmp_cli_links.h), and the rules file may then name link q as "l<q>" /
 * "!l<q>" (kmp_rules_parse_links).  Per shard and distinct buffer a context with the same tables and that buffer of every payload is
 * built as the variables above build theirs, one single-term rule per link is set on it, and kmpgpu_link_rows carries the rows into the
 * shard's own context (links_shards); the packets, alerts, flow-alerts, flow-bits and thresholds outputs then come from the shard's own
 * context, as without the variable.  Refused with a message on stderr and exit 1, before any GPU work: the variable together with
 * KMPGPU_DECODE, KMPGPU_HTTP_FIELD, KMPGPU_DNS_FIELD, KMPGPU_BASE64 (there the rows come from one buffer), KMPGPU_FLOW_SEAMS or
 * KMPGPU_FLOW_STREAMS; the variable without KMPGPU_RULES_FILE; a links file that does not parse (a negated or l term, a term out of
 * range); an unknown buffer; more than KMP_CLI_LINK_BUFFERS_MAX distinct buffers.
 *
 * KMPGPU_DNS_FIELD=qname[,tcp], together with at least one of KMPGPU_PACKETS_FILE, KMPGPU_ALERTS_FILE and KMPGPU_FLOW_ALERTS_FILE: these row
 * outputs are decided on the dotted name of the first question of the DNS message in every payload (kmpgpu_load_dns; the definition:
 * kmpgpu.h; ,tcp: a 2-byte length stands in front of every message), so that a rule that names `doubleclick.net` meets the queried name.
 * Per shard a second context on the shard's device gets the same tables as the shard's (upload_tables) and the name buffer of the shard's
 * arena, every payload (no message: an empty payload), so the payload numbers are the capture's.  stdout and KMPGPU_FLOWS_FILE are what
 * they are without the variable.  Refused with a message on stderr and exit 1, before any GPU work: any other value; the variable together
 * with KMPGPU_DECODE, KMPGPU_HTTP_FIELD, KMPGPU_BASE64, KMPGPU_OFFSETS_FILE, KMPGPU_EXPORT_FILE, KMPGPU_FLOW_SEAMS, KMPGPU_FLOW_STREAMS,
 * KMPGPU_FLOWBITS_FILE or KMPGPU_THRESHOLDS_FILE; the variable with none of the three row outputs.
 *
 * KMPGPU_TLS_FIELD=sni|alpn, together with at least one of KMPGPU_PACKETS_FILE, KMPGPU_ALERTS_FILE and KMPGPU_FLOW_ALERTS_FILE: these row
 * outputs are decided on the server name, or on the ALPN protocol list written as `h2,http/1.1`, of the TLS ClientHello in every payload
 * (kmpgpu_load_tls; the definition: kmpgpu.h), so that a rule that names `example.com` meets the server name and nothing else of the
 * connection.  Per shard a second context as KMPGPU_DNS_FIELD builds its own: every payload (no hello, or none with the field: an empty
 * payload), so the payload numbers are the capture's.  stdout and KMPGPU_FLOWS_FILE are what they are without the variable.  Refused with
 * a message on stderr and exit 1, before any GPU work and behind every other check: any other value; the variable together with
 * anything KMPGPU_DNS_FIELD does not go with, with KMPGPU_DNS_FIELD itself or with KMPGPU_LINKS_FILE (the links file has no tls: buffer
 * word; at the library a TLS buffer links like any other context); the variable with none of the three row outputs.
 *
 * KMPGPU_FLOW_STREAMS=<depth>, together with KMPGPU_FLOW_ALERTS_FILE: the flow alerts are decided on the reassembled streams.  A second
 * context on the shard's device gets the same tables as the shard's (upload_tables; the windows too: on a stream they mean "offset in the
 * connection's direction") and the payloads of every flow direction concatenated in capture order and cut to <depth> bytes
 * (kmpgpu_load_streams), its flows are built with the same flag (kmpgpu_flows_build: the flow numbers are the capture's), and the file
 * holds its kmpgpu_scan_flows(KMPGPU_ALERT_RULES, KMPGPU_FLOW_SCOPE_FLOW): a content however it was cut into segments, chains, byte
 * tests and expressions across segments.  <depth> is a decimal number in 1..1073741824, or one with k or m behind it (64k, 1m).
 * KMPGPU_STREAMS_FILE=<path>, together with KMPGPU_FLOW_STREAMS: one line per stream,
 * "stream,flow,dir,first_payload,last_payload,payloads,bytes,kept".  Refused with a message on stderr and exit 1, before any GPU work:
 * KMPGPU_FLOW_STREAMS without KMPGPU_FLOW_ALERTS_FILE, a value that is no depth, more than one shard, the variable together with
 * KMPGPU_FLOW_SEAMS (streams hold everything seams hold, up to the cut) or with KMPGPU_DECODE (decoded streams are not wired here; at the
 * library, kmpgpu_load_decoded over the stream context does it), KMPGPU_STREAMS_FILE without KMPGPU_FLOW_STREAMS or on a path that cannot
 * be written.  stdout is what it is without the variables.
 * KMPGPU_FLOW_STREAMS_ORDER=seq|capture (default capture), together with KMPGPU_FLOW_STREAMS: under seq the capture is read with its TCP
 * sequence numbers (kmp_arena_from_pcap_seq) and the streams of TCP flows are built in sequence order, retransmitted bytes dropped and
 * holes closed (kmpgpu_load_streams_ordered); KMPGPU_STREAMS_FILE then has the columns "tcp,gaps,gap_bytes,dup_bytes" behind the others,
 * and "bytes" counts the bytes kept.  Under capture every output is byte for byte what it is without the variable.  Refused: any other
 * value, the variable without KMPGPU_FLOW_STREAMS, and with KMPGPU_DEVICE_EXTRACT=1 (the device extractor keeps no sequence numbers).
 *
 * KMPGPU_FLOWBITS_FILE=<flow bits>, together with KMPGPU_RULES_FILE and KMPGPU_ALERTS_FILE: rule state carried along every flow's payloads
 * (kmpgpu_set_flowbits, kmpgpu_scan_flowbits; the file format is kmp_flowbits_parse's, kmphost.h: "<rule> set:<name> isset:<name> ...
 * noalert").  The payloads are grouped into flows (KMPGPU_FLOWS_DIRECTED=1: per direction) and the alerts file then holds the ALERT rows:
 * a rule's line for a payload where the rule matches it AND its tests hold on the state its flow's earlier payloads left; "payload,rule"
 * sorted as ever.  Message on stderr and exit 1, before any GPU work: the variable without the other two, more than one shard, the variable
 * together with KMPGPU_FLOW_ALERTS_FILE, KMPGPU_FLOW_SEAMS, KMPGPU_FLOW_STREAMS, KMPGPU_DECODE or KMPGPU_EXPORT_FILE (left for later), a
 * file that does not parse or whose bits form a cycle.  stdout is what it is without the variable.
 *
 * KMPGPU_THRESHOLDS_FILE=<thresholds>, together with KMPGPU_RULES_FILE and KMPGPU_ALERTS_FILE: a rule fires on the Nth hit per tracker in a
 * time window (kmpgpu_set_thresholds, kmpgpu_scan_thresholds; the file format is kmp_thresholds_parse's, kmphost.h: "<rule> by_src
 * at_least 5 60").  The timestamps are the capture's, in microseconds (kmp_arena_from_pcap_ts); the alerts file then holds the ALERT rows:
 * a rule's line for a payload where the rule matches it AND every threshold of the rule passes; "payload,rule" sorted as ever.  The
 * payloads are grouped into flows (KMPGPU_FLOWS_DIRECTED=1: per direction) only when a by_flow line is present.  Message on stderr and
 * exit 1, before any GPU work: the variable without the other two, more than one shard, the variable together with KMPGPU_FLOWBITS_FILE,
 * KMPGPU_FLOW_ALERTS_FILE, KMPGPU_FLOW_SEAMS, KMPGPU_FLOW_STREAMS, KMPGPU_DECODE or KMPGPU_EXPORT_FILE, with KMPGPU_DEVICE_EXTRACT=1 (the
 * device extractor keeps no timestamps), a file that does not parse.  stdout is what it is without the variable.
 *
 * KMPGPU_NOCASE=1: every pattern matches case-insensitively (ASCII letters; kmpgpu_set_patterns_flags), in the counts and in
 * the offsets file alike; the report prints every token as written in the pattern file.
 *
 * KMPGPU_WHOLE_PAYLOAD=1: a payload is matched up to its end instead of up to its first 0x00 (KMPGPU_OPT_WHOLE_PAYLOAD; not the
 * reference's behaviour), in the counts, the offsets file and the packets file alike; KMPGPU_STATS=1 prints which rule was used.
 * Unset or 0: the reference's rule, output as ever.
 */
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "kmpgpu.h"
#include "kmphost.h"
#include "kmp_cli_common.h"
#include "kmp_cli_decode.h"
#include "kmp_cli_base64.h"
#include "kmp_cli_fields.h"
#include "kmp_cli_dns.h"
#include "kmp_cli_tls.h"
#include "kmp_cli_links.h"
#include "kmp_cli_streams.h"
#include "kmp_cli_streams_order.h"

#ifndef KMP_CLI_OPENMP_FORM
#define KMP_CLI_OPENMP_FORM 0
#endif

#if KMP_CLI_OPENMP_FORM
#define PROG "./openmp_data"
#define ARGS "<file.pcap> <string.txt> thread_number [tcp/udp]"
#else
#define PROG "./serial"
#define ARGS "<file.pcap> <string.txt> [tcp/udp]"
#endif

/* What the command line and the environment ask for: filled once by load_options, read-only from then on. */
typedef struct cli_options {
    const char *pcap_path;
    int proto, shards;
    kmp_patterns pats;
    const uint8_t **pp;                     /* pp[i]: the bytes of pattern i */
    int whole_payload, nocase, device_extract, want_stats;
    const char *offsets_path, *packets_path, *rules_path, *alerts_path, *export_path, *flows_path, *flow_alerts_path;
    int flows_directed;                     /* KMPGPU_FLOWS_DIRECTED */
    uint32_t flow_seams;                    /* KMPGPU_FLOW_SEAMS: the reach, 0 without the variable */
    int decode;                             /* KMPGPU_DECODE: KMP_CLI_DECODE_* */
    int http_field;                         /* KMPGPU_HTTP_FIELD: KMP_CLI_FIELD_* */
    int dns_field, dns_tcp;                 /* KMPGPU_DNS_FIELD: KMP_CLI_DNS_*, and ",tcp" */
    int tls_field;                          /* KMPGPU_TLS_FIELD: KMP_CLI_TLS_* */
    unsigned base64_min_run;                /* KMPGPU_BASE64: min_run, 0 = not set */
    int base64_url;                         /* ... ,url */
    uint32_t flow_streams;                  /* KMPGPU_FLOW_STREAMS: the depth, 0 without the variable */
    const char *streams_path;               /* KMPGPU_STREAMS_FILE */
    int streams_order;                      /* KMPGPU_FLOW_STREAMS_ORDER: KMP_CLI_STREAMS_ORDER_* */
    int want_meta;                          /* header predicates or flows: the payloads' header fields go to the device */
    /* what every shard's context gets behind its patterns, in this order and before any rule is set */
    uint32_t *win_first, *win_last;         /* KMPGPU_WINDOWS_FILE (NULL: none) */
    kmp_relations relations;                /* KMPGPU_RELATIONS_FILE (n == 0: none) */
    kmp_chains chains;                      /* KMPGPU_CHAINS_FILE (n == 0: none) */
    kmp_headers headers;                    /* KMPGPU_HEADERS_FILE (n == 0: none) */
    kmp_bytetests bytetests;                /* KMPGPU_BYTETESTS_FILE (n == 0: none) */
    kmp_regexes regexes;                    /* KMPGPU_REGEX_FILE (n == 0: none) */
    const char *links_path;                 /* KMPGPU_LINKS_FILE */
    kmp_links links;                        /* ... its links (n == 0: none): link q is term l<q> of the rules */
    kmp_cli_link_buffer link_buf[KMP_CLI_LINK_BUFFERS_MAX];        /* ... the distinct buffers they name */
    int n_link_bufs;
    int *link_in;                           /* ... and link_in[q]: which of them link q is scanned in */
    kmp_rules rules;                        /* KMPGPU_RULES_FILE, set before the first output that needs them */
    const char *flowbits_path;              /* KMPGPU_FLOWBITS_FILE */
    kmp_flowbits flowbits;                  /* ... and its ops, set behind the rules (n == 0: none) */
    const char *thresholds_path;            /* KMPGPU_THRESHOLDS_FILE */
    kmp_thresholds thresholds;              /* ... and its thresholds, set behind the rules (n == 0: none) */
    int thresholds_by_flow, thresholds_by_addr;       /* some line is by_flow; by_src or by_dst */
} cli_options;

/* The capture in host memory -- as payloads, or with KMPGPU_DEVICE_EXTRACT=1 as raw frames -- and when it got there. */
typedef struct capture {
    kmp_arena arena;
    kmp_frames frames;
    kmp_pkt_meta *meta;                     /* beside the arena where header predicates are set: its payloads' header fields */
    uint32_t *seq;                          /* ... and under KMPGPU_FLOW_STREAMS_ORDER=seq their TCP sequence numbers */
    uint64_t *ts;                           /* ... and under KMPGPU_THRESHOLDS_FILE their capture times in microseconds */
    double t_load0, t_loaded, t_warm;
} capture;

/* One GPU shard: a contiguous range of the payloads (or, with KMPGPU_DEVICE_EXTRACT=1, of the frames). */
typedef struct shard_job {
    const cli_options *opt;
    const capture *cap;
    int device, threaded, rc;
    uint64_t lo, cnt;                       /* first unit and number of units of this shard */
    kmpgpu_ctx *ctx;
    kmpgpu_timing t;
    uint64_t n_payloads, payload_bytes;     /* what the context holds (kmpgpu_arena_info) */
    uint64_t payload_lo;                    /* index of the shard's first payload among all payloads */
    uint64_t *reb;
    const char *what;
    char err[512];
    pthread_t thread;
} shard_job;

/* The shards of a run and what they found. */
typedef struct cli_run {
    int ndev, shards, reduce_rccl, rules_set;
    shard_job *job;
    kmpgpu_ctx **ctxs;                      /* ctxs[r] = job[r].ctx */
    kmpgpu_ctx **rows;                      /* rows[r]: the context the row outputs of shard r come from -- ctxs[r], or with KMPGPU_DECODE its decoding, with KMPGPU_HTTP_FIELD its field buffer, with KMPGPU_BASE64 its base64 decoding, with KMPGPU_DNS_FIELD its name buffer, with KMPGPU_TLS_FIELD its server-name or ALPN buffer */
    kmpgpu_comm *comm;
    uint64_t *own, *counts;                 /* own[r * n_patterns + i]: shard r's count of pattern i; counts[i]: the total */
    double kernel_ms;
    uint64_t eff_bytes;
} cli_run;

static void usage(const char *head)
{
    printf("%s " PROG " " ARGS "\n", head);                                 /* "USAGE": serial.c:43, openmp_data.c:46; "USAGE:": serial.c:49, openmp_data.c:52 */
    exit(1);
}

/* an output file that cannot be written ends the run before any GPU work; one that can starts empty */
static void probe_writable(const char *var, const char *path)
{
    if (!path) return;
    FILE *fp = fopen(path, "w");
    if (!fp) { perror(var); exit(1); }
    fclose(fp);
}

static void needs_rules_and_alerts(const char *var, const cli_options *opt)
{
    if (opt->rules_path && opt->alerts_path) return;
    fprintf(stderr, "%s goes together with KMPGPU_RULES_FILE and KMPGPU_ALERTS_FILE: %s is not set\n", var, opt->rules_path ? "KMPGPU_ALERTS_FILE" : "KMPGPU_RULES_FILE");
    exit(1);
}

/* The command line, the pattern file and every environment variable, each read once; the files that say what to look for are parsed and
 * the export path is probed.  Whatever is wrong ends the run here with exit code 1, before anything touches the GPU. */
static void load_options(int argc, char *argv[], cli_options *opt)
{
    memset(opt, 0, sizeof *opt);
    opt->proto = KMP_PROTO_UDP;                                             /* serial.c:31 */
    opt->shards = 1;
    if (argc != 3 + KMP_CLI_OPENMP_FORM && argc != 4 + KMP_CLI_OPENMP_FORM) usage("USAGE:");       /* serial.c:33, openmp_data.c:35 */
#if KMP_CLI_OPENMP_FORM
    opt->shards = atoi(argv[3]);                                            /* openmp_data.c:38 */
    if (opt->shards < 1) opt->shards = 1;
#endif
    if (argc == 4 + KMP_CLI_OPENMP_FORM && !parse_proto(argv[argc - 1], &opt->proto)) usage("USAGE");
    opt->pcap_path = argv[1];

    const int rc = kmp_patterns_load(argv[2], &opt->pats);                  /* serial.c:54-87 */
    if (rc == KMPHOST_EIO) {
        perror("error opening file: ");                                     /* serial.c:61 */
        exit(1);
    }
    if (rc) {
        fprintf(stderr, "error reading pattern file: %s\n", rc == KMPHOST_ETOKEN ? "token longer than 99 bytes" : "out of memory");
        exit(1);
    }
    const uint32_t n = opt->pats.n;
    opt->pp = (const uint8_t **)malloc(sizeof(uint8_t *) * (n ? n : 1));
    for (uint32_t i = 0; i < n; i++) opt->pp[i] = opt->pats.blob + opt->pats.off[i];

    opt->whole_payload = env_flag("KMPGPU_WHOLE_PAYLOAD");
    opt->nocase = env_flag("KMPGPU_NOCASE");
    opt->device_extract = env_device_extract();
    /* KMPGPU_STATS=1: also report the bytes up to the first NUL of every payload (what strlen bounds, serial.c:191);
     * one extra pass over the arena, so it is opt-in and the "Elapsed time" line of a plain run stays comparable */
    opt->want_stats = env_stats();
    opt->offsets_path = env_path("KMPGPU_OFFSETS_FILE");
    opt->packets_path = env_path("KMPGPU_PACKETS_FILE");
    opt->rules_path = env_path("KMPGPU_RULES_FILE");
    opt->alerts_path = env_path("KMPGPU_ALERTS_FILE");
    opt->export_path = env_path("KMPGPU_EXPORT_FILE");
    opt->flows_path = env_path("KMPGPU_FLOWS_FILE");
    opt->flow_alerts_path = env_path("KMPGPU_FLOW_ALERTS_FILE");
    opt->flows_directed = env_flag("KMPGPU_FLOWS_DIRECTED");
    const char *relations_path = env_path("KMPGPU_RELATIONS_FILE"), *chains_path = env_path("KMPGPU_CHAINS_FILE"), *headers_path = env_path("KMPGPU_HEADERS_FILE"), *bytetests_path = env_path("KMPGPU_BYTETESTS_FILE"), *regex_path = env_path("KMPGPU_REGEX_FILE"), *windows_path = env_path("KMPGPU_WINDOWS_FILE");

    /* the content rules (an export takes the rules' any[] without an alerts file) */
    if ((opt->rules_path != NULL) != (opt->alerts_path != NULL) && !(opt->rules_path && (opt->export_path || opt->flow_alerts_path))) {
        fprintf(stderr, "KMPGPU_RULES_FILE and KMPGPU_ALERTS_FILE go together: %s is not set\n", opt->rules_path ? "KMPGPU_ALERTS_FILE" : "KMPGPU_RULES_FILE");
        exit(1);
    }
    /* the relations, the chains, the header predicates, the byte tests and the expressions, which the rules may name */
    char err[256];
    _Static_assert(sizeof err >= KMP_RELATIONS_ERRBUF && sizeof err >= KMP_CHAINS_ERRBUF && sizeof err >= KMP_RULES_ERRBUF && sizeof err >= KMP_WINDOWS_ERRBUF && sizeof err >= KMP_HEADERS_ERRBUF && sizeof err >= KMP_BYTETESTS_ERRBUF && sizeof err >= KMP_REGEXES_ERRBUF,
                   "room for every parser's message");
    if (relations_path) {
        needs_rules_and_alerts("KMPGPU_RELATIONS_FILE", opt);
        if (kmp_relations_parse(relations_path, n, &opt->relations, err)) {
            fprintf(stderr, "error reading relations file %s: %s\n", relations_path, err);
            exit(1);
        }
    }
    if (chains_path) {
        needs_rules_and_alerts("KMPGPU_CHAINS_FILE", opt);
        if (kmp_chains_parse(chains_path, n, &opt->chains, err)) {
            fprintf(stderr, "error reading chains file %s: %s\n", chains_path, err);
            exit(1);
        }
    }
    if (headers_path) {
        needs_rules_and_alerts("KMPGPU_HEADERS_FILE", opt);
        if (kmp_headers_parse(headers_path, &opt->headers, err)) {
            fprintf(stderr, "error reading headers file %s: %s\n", headers_path, err);
            exit(1);
        }
    }
    if (bytetests_path) {
        /* a term of the rules, for the alerts per payload or per flow (or both) */
        if (!opt->rules_path || (!opt->alerts_path && !opt->flow_alerts_path)) {
            fprintf(stderr, "KMPGPU_BYTETESTS_FILE goes together with KMPGPU_RULES_FILE and KMPGPU_ALERTS_FILE or KMPGPU_FLOW_ALERTS_FILE: %s is not set\n",
                    opt->rules_path ? "neither of the two" : "KMPGPU_RULES_FILE");
            exit(1);
        }
        if (kmp_bytetests_parse(bytetests_path, n, &opt->bytetests, err)) {
            fprintf(stderr, "error reading byte tests file %s: %s\n", bytetests_path, err);
            exit(1);
        }
    }
    if (regex_path) {
        /* a term of the rules, for the alerts per payload or per flow (or both) */
        if (!opt->rules_path || (!opt->alerts_path && !opt->flow_alerts_path)) {
            fprintf(stderr, "KMPGPU_REGEX_FILE goes together with KMPGPU_RULES_FILE and KMPGPU_ALERTS_FILE or KMPGPU_FLOW_ALERTS_FILE: %s is not set\n",
                    opt->rules_path ? "neither of the two" : "KMPGPU_RULES_FILE");
            exit(1);
        }
        if (kmp_regexes_parse(regex_path, n, &opt->regexes, err)) {
            fprintf(stderr, "error reading expressions file %s: %s\n", regex_path, err);
            exit(1);
        }
    }
    /* the links: rows of other buffers of the same payloads, which the rules may name as l<q> */
    opt->links_path = env_path("KMPGPU_LINKS_FILE");
    if (opt->links_path) {
        static const char *const not_with[][2] = {
            {"KMPGPU_DECODE", "there the rows come from one buffer; a line 'decode:percent <term>' links it"},
            {"KMPGPU_HTTP_FIELD", "there the rows come from one buffer; a line 'http:<field> <term>' links it"},
            {"KMPGPU_DNS_FIELD", "there the rows come from one buffer; a line 'dns:qname <term>' links it"},
            {"KMPGPU_BASE64", "there the rows come from one buffer; a line 'base64:<min_run> <term>' links it"},
            {"KMPGPU_FLOW_SEAMS", "seams are numbered by themselves, links in this program by the capture's payloads"},
            {"KMPGPU_FLOW_STREAMS", "streams are numbered by themselves, links in this program by the capture's payloads"}};
        _Static_assert(sizeof err >= KMP_LINKS_ERRBUF, "room for the links parser's message");
        for (size_t i = 0; i < sizeof not_with / sizeof not_with[0]; i++)
            if (env_path(not_with[i][0])) {
                fprintf(stderr, "KMPGPU_LINKS_FILE does not go together with %s: %s\n", not_with[i][0], not_with[i][1]);
                exit(1);
            }
        if (!opt->rules_path) {
            fprintf(stderr, "KMPGPU_LINKS_FILE goes together with KMPGPU_RULES_FILE: a link is a term l<q> of a rule\n");
            exit(1);
        }
        if (kmp_links_parse(opt->links_path, n, opt->relations.n, opt->chains.n, opt->headers.n, opt->bytetests.n, opt->regexes.n, &opt->links, err)) {
            fprintf(stderr, "error reading links file %s: %s\n", opt->links_path, err);
            exit(1);
        }
        opt->link_in = (int *)malloc(sizeof(int) * (opt->links.n ? opt->links.n : 1));
        for (uint32_t q = 0; q < opt->links.n; q++) {
            kmp_cli_link_buffer b;
            if (!kmp_cli_parse_link_buffer(opt->links.buffer[q], &b)) {
                fprintf(stderr, "KMPGPU_LINKS_FILE: link %u: '%s' is no buffer (http:method|raw_uri|uri|status|headers|body, dns:qname[,tcp], decode:percent[+plus], base64:<min_run>[,url])\n",
                        q, opt->links.buffer[q]);
                exit(1);
            }
            int at = 0;
            while (at < opt->n_link_bufs && !kmp_cli_link_buffer_same(&opt->link_buf[at], &b)) at++;
            if (at == opt->n_link_bufs) {
                if (at == KMP_CLI_LINK_BUFFERS_MAX) {
                    fprintf(stderr, "KMPGPU_LINKS_FILE: link %u: '%s' is buffer %d: at most %d distinct buffers\n", q, opt->links.buffer[q], at + 1, KMP_CLI_LINK_BUFFERS_MAX);
                    exit(1);
                }
                opt->link_buf[opt->n_link_bufs++] = b;
            }
            opt->link_in[q] = at;
        }
    }
    if (opt->rules_path && kmp_rules_parse_links(opt->rules_path, n, opt->relations.n, opt->chains.n, opt->headers.n, opt->bytetests.n, opt->regexes.n, opt->links.n, &opt->rules, err)) {
        fprintf(stderr, "error reading rules file %s: %s\n", opt->rules_path, err);
        exit(1);
    }
    /* flow bits: they change what the alerts file holds and nothing else; one shard, whose payloads are grouped into flows */
    opt->flowbits_path = env_path("KMPGPU_FLOWBITS_FILE");
    if (opt->flowbits_path) {
        static const char *const not_with[][2] = {
            {"KMPGPU_FLOW_ALERTS_FILE", "the rules per flow know no flow bits"}, {"KMPGPU_FLOW_SEAMS", "seams carry no state"},
            {"KMPGPU_FLOW_STREAMS", "streams carry no state"}, {"KMPGPU_DECODE", "decoded payloads are grouped into no flows in this program"},
            {"KMPGPU_EXPORT_FILE", "the export selects by the rules without their flow bits"}};
        needs_rules_and_alerts("KMPGPU_FLOWBITS_FILE", opt);
        if (opt->shards > 1) {
            fprintf(stderr, "KMPGPU_FLOWBITS_FILE needs one shard, thread_number is %d: a flow would be cut at a shard's edge\n", opt->shards);
            exit(1);
        }
        for (size_t i = 0; i < sizeof not_with / sizeof not_with[0]; i++)
            if (env_path(not_with[i][0])) {
                fprintf(stderr, "KMPGPU_FLOWBITS_FILE does not go together with %s: %s\n", not_with[i][0], not_with[i][1]);
                exit(1);
            }
        _Static_assert(sizeof err >= KMP_FLOWBITS_ERRBUF, "room for the flow bits parser's message");
        if (kmp_flowbits_parse(opt->flowbits_path, opt->rules.n, &opt->flowbits, err)) {
            fprintf(stderr, "error reading flow bits file %s: %s\n", opt->flowbits_path, err);
            exit(1);
        }
    }
    /* rate thresholds: they too change what the alerts file holds and nothing else; one shard, whose timestamps come from the capture */
    opt->thresholds_path = env_path("KMPGPU_THRESHOLDS_FILE");
    if (opt->thresholds_path) {
        static const char *const not_with[][2] = {
            {"KMPGPU_FLOWBITS_FILE", "thresholds over flow-bit alerts are not defined"}, {"KMPGPU_FLOW_ALERTS_FILE", "the rules per flow know no thresholds"},
            {"KMPGPU_FLOW_SEAMS", "seams have no time"}, {"KMPGPU_FLOW_STREAMS", "streams have no time"},
            {"KMPGPU_DECODE", "decoded payloads keep no timestamps in this program"}, {"KMPGPU_EXPORT_FILE", "the export selects by the rules without their thresholds"}};
        needs_rules_and_alerts("KMPGPU_THRESHOLDS_FILE", opt);
        if (opt->shards > 1) {
            fprintf(stderr, "KMPGPU_THRESHOLDS_FILE needs one shard, thread_number is %d: a tracker's window would be cut at a shard's edge\n", opt->shards);
            exit(1);
        }
        for (size_t i = 0; i < sizeof not_with / sizeof not_with[0]; i++)
            if (env_path(not_with[i][0])) {
                fprintf(stderr, "KMPGPU_THRESHOLDS_FILE does not go together with %s: %s\n", not_with[i][0], not_with[i][1]);
                exit(1);
            }
        if (opt->device_extract) {
            fprintf(stderr, "KMPGPU_THRESHOLDS_FILE does not go together with KMPGPU_DEVICE_EXTRACT=1: the device extractor keeps no timestamps\n");
            exit(1);
        }
        _Static_assert(sizeof err >= KMP_THRESHOLDS_ERRBUF, "room for the thresholds parser's message");
        if (kmp_thresholds_parse(opt->thresholds_path, opt->rules.n, &opt->thresholds, err)) {
            fprintf(stderr, "error reading thresholds file %s: %s\n", opt->thresholds_path, err);
            exit(1);
        }
        for (uint32_t q = 0; q < opt->thresholds.n; q++) {
            if (opt->thresholds.thr[q].track == KMP_THR_BY_FLOW) opt->thresholds_by_flow = 1;
            if (opt->thresholds.thr[q].track == KMP_THR_BY_SRC || opt->thresholds.thr[q].track == KMP_THR_BY_DST) opt->thresholds_by_addr = 1;
        }
    }
    /* the offset windows likewise */
    if (windows_path) {
        if (!opt->offsets_path && !opt->packets_path && !opt->alerts_path && !opt->export_path) {
            fprintf(stderr, "KMPGPU_WINDOWS_FILE has no effect without KMPGPU_OFFSETS_FILE, KMPGPU_PACKETS_FILE, KMPGPU_EXPORT_FILE or KMPGPU_RULES_FILE + KMPGPU_ALERTS_FILE\n");
            exit(1);
        }
        opt->win_first = (uint32_t *)malloc(sizeof(uint32_t) * (n ? n : 1));
        opt->win_last = (uint32_t *)malloc(sizeof(uint32_t) * (n ? n : 1));
        if (!opt->win_first || !opt->win_last) { fprintf(stderr, "error reading windows file %s: out of memory\n", windows_path); exit(1); }
        if (kmp_windows_parse(windows_path, n, opt->win_first, opt->win_last, err)) {
            fprintf(stderr, "error reading windows file %s: %s\n", windows_path, err);
            exit(1);
        }
    }
    /* flows: one shard, rules for the flow alerts, and both files started empty */
    if (opt->flows_path || opt->flow_alerts_path) {
        if (opt->shards > 1) {
            fprintf(stderr, "KMPGPU_FLOWS_FILE and KMPGPU_FLOW_ALERTS_FILE need one shard, thread_number is %d: a flow would be cut at a shard's edge\n", opt->shards);
            exit(1);
        }
        if (opt->flow_alerts_path && !opt->rules_path) {
            fprintf(stderr, "KMPGPU_FLOW_ALERTS_FILE goes together with KMPGPU_RULES_FILE: it is not set\n");
            exit(1);
        }
        probe_writable("KMPGPU_FLOWS_FILE", opt->flows_path);
        probe_writable("KMPGPU_FLOW_ALERTS_FILE", opt->flow_alerts_path);
    }
    /* seams: they change what the flow alerts file holds and nothing else */
    const char *seams_env = env_path("KMPGPU_FLOW_SEAMS");
    if (seams_env) {
        if (!opt->flow_alerts_path) {
            fprintf(stderr, "KMPGPU_FLOW_SEAMS goes together with KMPGPU_FLOW_ALERTS_FILE: it is not set\n");
            exit(1);
        }
        char *end = NULL;
        const long reach = strtol(seams_env, &end, 10);
        if (end == seams_env || *end || reach < 1 || reach > KMPGPU_MAX_PATTERN_LEN - 1) {
            fprintf(stderr, "KMPGPU_FLOW_SEAMS is \"%s\": a reach of 1..%d bytes is needed\n", seams_env, KMPGPU_MAX_PATTERN_LEN - 1);
            exit(1);
        }
        opt->flow_seams = (uint32_t)reach;
    }
    /* the decoded buffer: it changes what the row outputs hold and nothing else */
    const char *decode_env = env_path("KMPGPU_DECODE");
    if (decode_env) {
        if (!kmp_cli_parse_decode(decode_env, &opt->decode)) {
            fprintf(stderr, "KMPGPU_DECODE is \"%s\": percent or percent+plus is needed\n", decode_env);
            exit(1);
        }
        if (opt->offsets_path) {
            fprintf(stderr, "KMPGPU_DECODE does not go together with KMPGPU_OFFSETS_FILE: offsets in decoded payloads are not mapped back to the capture's\n");
            exit(1);
        }
        if (opt->export_path) {
            fprintf(stderr, "KMPGPU_DECODE does not go together with KMPGPU_EXPORT_FILE: the export selects and writes the payloads as captured\n");
            exit(1);
        }
        if (opt->flow_seams) {
            fprintf(stderr, "KMPGPU_DECODE does not go together with KMPGPU_FLOW_SEAMS: decoded seams do not exist\n");
            exit(1);
        }
        if (!opt->packets_path && !opt->alerts_path && !opt->flow_alerts_path) {
            fprintf(stderr, "KMPGPU_DECODE has no effect without KMPGPU_PACKETS_FILE, KMPGPU_ALERTS_FILE or KMPGPU_FLOW_ALERTS_FILE\n");
            exit(1);
        }
    }
    /* streams: they change what the flow alerts file holds, and write a file of their own */
    const char *streams_env = env_path("KMPGPU_FLOW_STREAMS");
    opt->streams_path = env_path("KMPGPU_STREAMS_FILE");
    if (streams_env) {
        if (!opt->flow_alerts_path) {
            fprintf(stderr, "KMPGPU_FLOW_STREAMS goes together with KMPGPU_FLOW_ALERTS_FILE: it is not set\n");
            exit(1);
        }
        if (!kmp_cli_parse_depth(streams_env, &opt->flow_streams)) {
            fprintf(stderr, "KMPGPU_FLOW_STREAMS is \"%s\": a depth of 1..%u bytes is needed\n", streams_env, KMP_CLI_STREAM_DEPTH_MAX);
            exit(1);
        }
        if (opt->flow_seams) {
            fprintf(stderr, "KMPGPU_FLOW_STREAMS does not go together with KMPGPU_FLOW_SEAMS: streams hold everything seams hold, up to the cut\n");
            exit(1);
        }
        if (opt->decode) {
            fprintf(stderr, "KMPGPU_FLOW_STREAMS does not go together with KMPGPU_DECODE: decoded streams are not wired in this program\n");
            exit(1);
        }
    }
    if (opt->streams_path) {
        if (!opt->flow_streams) {
            fprintf(stderr, "KMPGPU_STREAMS_FILE goes together with KMPGPU_FLOW_STREAMS: it is not set\n");
            exit(1);
        }
        probe_writable("KMPGPU_STREAMS_FILE", opt->streams_path);
    }
    const char *order_env = env_path("KMPGPU_FLOW_STREAMS_ORDER");
    if (order_env) {
        if (!kmp_cli_parse_streams_order(order_env, &opt->streams_order)) {
            fprintf(stderr, "KMPGPU_FLOW_STREAMS_ORDER is \"%s\": seq or capture is needed\n", order_env);
            exit(1);
        }
        if (!opt->flow_streams) {
            fprintf(stderr, "KMPGPU_FLOW_STREAMS_ORDER goes together with KMPGPU_FLOW_STREAMS: it is not set\n");
            exit(1);
        }
        if (opt->streams_order == KMP_CLI_STREAMS_ORDER_SEQ && opt->device_extract) {
            fprintf(stderr, "KMPGPU_FLOW_STREAMS_ORDER=seq does not go together with KMPGPU_DEVICE_EXTRACT=1: the device extractor keeps no sequence numbers\n");
            exit(1);
        }
    }
    /* the field buffer: it changes what the row outputs hold and nothing else */
    const char *field_env = env_path("KMPGPU_HTTP_FIELD");
    if (field_env) {
        static const char *const not_with[][2] = {
            {"KMPGPU_DECODE", "uri is the percent-decoded field, every other field is taken as captured"},
            {"KMPGPU_OFFSETS_FILE", "offsets in a field are not mapped back to the capture's"},
            {"KMPGPU_EXPORT_FILE", "the export selects and writes the payloads as captured"},
            {"KMPGPU_FLOW_SEAMS", "seams of fields do not exist"},
            {"KMPGPU_FLOW_STREAMS", "fields of streams are not wired in this program"},
            {"KMPGPU_FLOWBITS_FILE", "flow bits over a field buffer are not wired in this program"},
            {"KMPGPU_THRESHOLDS_FILE", "a field buffer keeps no timestamps in this program"}};
        if (!kmp_cli_parse_field(field_env, &opt->http_field)) {
            fprintf(stderr, "KMPGPU_HTTP_FIELD is \"%s\": method, raw_uri, uri, status, headers or body is needed\n", field_env);
            exit(1);
        }
        for (size_t i = 0; i < sizeof not_with / sizeof not_with[0]; i++)
            if (env_path(not_with[i][0])) {
                fprintf(stderr, "KMPGPU_HTTP_FIELD does not go together with %s: %s\n", not_with[i][0], not_with[i][1]);
                exit(1);
            }
        if (!opt->packets_path && !opt->alerts_path && !opt->flow_alerts_path) {
            fprintf(stderr, "KMPGPU_HTTP_FIELD has no effect without KMPGPU_PACKETS_FILE, KMPGPU_ALERTS_FILE or KMPGPU_FLOW_ALERTS_FILE\n");
            exit(1);
        }
    }
    /* the base64-decoded buffer: it changes what the row outputs hold and nothing else */
    const char *base64_env = env_path("KMPGPU_BASE64");
    if (base64_env) {
        static const char *const not_with[][2] = {
            {"KMPGPU_DECODE", "one decoding per run; at the library, kmpgpu_load_decoded over the base64 context does both"},
            {"KMPGPU_HTTP_FIELD", "base64 in a field buffer is not wired in this program"},
            {"KMPGPU_OFFSETS_FILE", "offsets in decoded payloads are not mapped back to the capture's"},
            {"KMPGPU_EXPORT_FILE", "the export selects and writes the payloads as captured"},
            {"KMPGPU_FLOW_SEAMS", "decoded seams do not exist"},
            {"KMPGPU_FLOW_STREAMS", "base64 in streams is not wired in this program"},
            {"KMPGPU_FLOWBITS_FILE", "flow bits over base64-decoded payloads are not wired in this program"},
            {"KMPGPU_THRESHOLDS_FILE", "base64-decoded payloads keep no timestamps in this program"}};
        if (!kmp_cli_parse_base64(base64_env, &opt->base64_min_run, &opt->base64_url)) {
            fprintf(stderr, "KMPGPU_BASE64 is \"%s\": <min_run> or <min_run>,url with a min_run of %u..%u is needed\n", base64_env, KMP_CLI_BASE64_MIN_RUN_LO,
                    KMP_CLI_BASE64_MIN_RUN_HI);
            exit(1);
        }
        for (size_t i = 0; i < sizeof not_with / sizeof not_with[0]; i++)
            if (env_path(not_with[i][0])) {
                fprintf(stderr, "KMPGPU_BASE64 does not go together with %s: %s\n", not_with[i][0], not_with[i][1]);
                exit(1);
            }
        if (!opt->packets_path && !opt->alerts_path && !opt->flow_alerts_path) {
            fprintf(stderr, "KMPGPU_BASE64 has no effect without KMPGPU_PACKETS_FILE, KMPGPU_ALERTS_FILE or KMPGPU_FLOW_ALERTS_FILE\n");
            exit(1);
        }
    }
    /* the DNS name buffer: it changes what the row outputs hold and nothing else */
    const char *dns_env = env_path("KMPGPU_DNS_FIELD");
    if (dns_env) {
        static const char *const not_with[][2] = {
            {"KMPGPU_DECODE", "a name is taken as it is on the wire; at the library, kmpgpu_load_decoded over the name context decodes it"},
            {"KMPGPU_HTTP_FIELD", "one buffer per run"},
            {"KMPGPU_BASE64", "base64 in a name buffer is not wired in this program"},
            {"KMPGPU_OFFSETS_FILE", "offsets in a name are not mapped back to the capture's"},
            {"KMPGPU_EXPORT_FILE", "the export selects and writes the payloads as captured"},
            {"KMPGPU_FLOW_SEAMS", "seams of names do not exist"},
            {"KMPGPU_FLOW_STREAMS", "names of streams are not wired in this program"},
            {"KMPGPU_FLOWBITS_FILE", "flow bits over a name buffer are not wired in this program"},
            {"KMPGPU_THRESHOLDS_FILE", "a name buffer keeps no timestamps in this program"}};
        if (!kmp_cli_parse_dns(dns_env, &opt->dns_field, &opt->dns_tcp)) {
            fprintf(stderr, "KMPGPU_DNS_FIELD is \"%s\": qname or qname,tcp is needed\n", dns_env);
            exit(1);
        }
        for (size_t i = 0; i < sizeof not_with / sizeof not_with[0]; i++)
            if (env_path(not_with[i][0])) {
                fprintf(stderr, "KMPGPU_DNS_FIELD does not go together with %s: %s\n", not_with[i][0], not_with[i][1]);
                exit(1);
            }
        if (!opt->packets_path && !opt->alerts_path && !opt->flow_alerts_path) {
            fprintf(stderr, "KMPGPU_DNS_FIELD has no effect without KMPGPU_PACKETS_FILE, KMPGPU_ALERTS_FILE or KMPGPU_FLOW_ALERTS_FILE\n");
            exit(1);
        }
    }
    /* the TLS server-name or ALPN buffer: it changes what the row outputs hold and nothing else.  Behind every other check. */
    const char *tls_env = env_path("KMPGPU_TLS_FIELD");
    if (tls_env) {
        static const char *const not_with[][2] = {
            {"KMPGPU_DECODE", "a field is taken as it is on the wire; at the library, kmpgpu_load_decoded over the TLS context decodes it"},
            {"KMPGPU_HTTP_FIELD", "one buffer per run"},
            {"KMPGPU_DNS_FIELD", "one buffer per run"},
            {"KMPGPU_BASE64", "base64 in a TLS buffer is not wired in this program"},
            {"KMPGPU_LINKS_FILE", "the links file has no tls: buffer word; at the library, kmpgpu_link_rows links a TLS buffer like any other context"},
            {"KMPGPU_OFFSETS_FILE", "offsets in a field are not mapped back to the capture's"},
            {"KMPGPU_EXPORT_FILE", "the export selects and writes the payloads as captured"},
            {"KMPGPU_FLOW_SEAMS", "seams of TLS fields do not exist"},
            {"KMPGPU_FLOW_STREAMS", "TLS fields of streams are not wired in this program"},
            {"KMPGPU_FLOWBITS_FILE", "flow bits over a TLS buffer are not wired in this program"},
            {"KMPGPU_THRESHOLDS_FILE", "a TLS buffer keeps no timestamps in this program"}};
        if (!kmp_cli_parse_tls(tls_env, &opt->tls_field)) {
            fprintf(stderr, "KMPGPU_TLS_FIELD is \"%s\": sni or alpn is needed\n", tls_env);
            exit(1);
        }
        for (size_t i = 0; i < sizeof not_with / sizeof not_with[0]; i++)
            if (env_path(not_with[i][0])) {
                fprintf(stderr, "KMPGPU_TLS_FIELD does not go together with %s: %s\n", not_with[i][0], not_with[i][1]);
                exit(1);
            }
        if (!opt->packets_path && !opt->alerts_path && !opt->flow_alerts_path) {
            fprintf(stderr, "KMPGPU_TLS_FIELD has no effect without KMPGPU_PACKETS_FILE, KMPGPU_ALERTS_FILE or KMPGPU_FLOW_ALERTS_FILE\n");
            exit(1);
        }
    }
    opt->want_meta = opt->headers.n || opt->flows_path || opt->flow_alerts_path || opt->flowbits.n || opt->thresholds_by_flow || opt->thresholds_by_addr;
    /* the export starts as a capture without frames: a path that cannot be written ends the run here */
    if (opt->export_path && kmp_write_udp_pcap_part(opt->export_path, 0, NULL, NULL, NULL, 0, 0)) {
        perror("KMPGPU_EXPORT_FILE");
        exit(1);
    }
}

static void free_options(cli_options *opt)
{
    free(opt->pp);
    kmp_patterns_free(&opt->pats);
    kmp_rules_free(&opt->rules);
    kmp_links_free(&opt->links);
    free(opt->link_in);
    kmp_relations_free(&opt->relations);
    kmp_chains_free(&opt->chains);
    kmp_headers_free(&opt->headers);
    kmp_bytetests_free(&opt->bytetests);
    kmp_regexes_free(&opt->regexes);
    kmp_flowbits_free(&opt->flowbits);
    kmp_thresholds_free(&opt->thresholds);
    free(opt->win_first); free(opt->win_last);
}

/* The HIP runtime takes 0.2-0.3 s to come up.  It does so on a side thread while the main thread maps, indexes
 * and extracts the capture; the two meet before the first context is created. */
static void *warm_gpu(void *arg)
{
    (void)arg;
    if (kmpgpu_device_count() > 0) {
        kmpgpu_ctx *w = NULL;
        if (kmpgpu_init(&w, 0) == 0) kmpgpu_destroy(w);
    }
    return NULL;
}

static void load_capture(const cli_options *opt, capture *cap)
{
    memset(cap, 0, sizeof *cap);
    pthread_t warm;
    const int warming = pthread_create(&warm, NULL, warm_gpu, NULL) == 0;
    cap->t_load0 = now_s();
    char errbuf[KMP_PCAP_ERRBUF];
    int rc;
    /* One-shot buffers stay in ordinary memory: pinning 1.5 GB costs 0.22 s and unpinning 0.15 s, while the
     * host-to-device copy runs at PCIe speed from pageable memory and even straight from the mapped file on the
     * MI355X hosts (profiles/r01_h2d_probe.txt).  Pinned buffers pay off where they are reused (bin/openmp_task). */
    if (opt->device_extract)
        rc = kmp_frames_from_pcap(opt->pcap_path, NULL, NULL, &cap->frames, errbuf);
    else if (opt->streams_order == KMP_CLI_STREAMS_ORDER_SEQ)               /* (streams go with flow alerts: the header fields are wanted too) */
        rc = kmp_arena_from_pcap_seq(opt->pcap_path, opt->proto, NULL, NULL, &cap->arena, errbuf, &cap->meta, &cap->seq);
    else if (opt->thresholds.n)                                             /* the same arena, and every payload's capture time */
        rc = kmp_arena_from_pcap_ts(opt->pcap_path, opt->proto, NULL, NULL, &cap->arena, errbuf, opt->want_meta ? &cap->meta : NULL, &cap->ts);
    else if (opt->want_meta)                                                /* the same arena, and the header fields the predicates and the flows read */
        rc = kmp_arena_from_pcap_meta(opt->pcap_path, opt->proto, NULL, NULL, &cap->arena, errbuf, &cap->meta);
    else
        rc = kmp_arena_from_pcap(opt->pcap_path, opt->proto, NULL, NULL, &cap->arena, errbuf);                /* serial.c:91-141 */
    cap->t_loaded = now_s();
    if (warming) pthread_join(warm, NULL);                                  /* the runtime is up (or there is none: reported by main) */
    cap->t_warm = now_s();
    if (rc == KMPHOST_EIO || rc == KMPHOST_EFORMAT) {
        fprintf(stderr, "error reading pcap file: %s\n", errbuf);           /* serial.c:93 */
        exit(1);
    }
    if (rc) {
        fprintf(stderr, "error building the payload arena: %s\n", errbuf[0] ? errbuf : kmpgpu_last_error());
        exit(2);
    }
}

static void *shard_fail(shard_job *j, const char *what)
{
    j->rc = 1; j->what = what;
    snprintf(j->err, sizeof j->err, "%s", kmpgpu_last_error());            /* the error text is per thread */
    return NULL;
}

/* What a context of the run scans with, in this order and before any rule is set: the patterns with the environment's text rule and
 * case rule, the windows, relations, chains, header predicates, byte tests and expressions.  Every shard's context and, with
 * KMPGPU_DECODE, its decoding pass through here.  Returns NULL, or the name of the call that failed. */
static const char *upload_tables(kmpgpu_ctx *ctx, const cli_options *o)
{
    if (set_patterns_env(ctx, o->pp, o->pats.len, o->pats.n, o->whole_payload, o->nocase)) return "kmpgpu_set_patterns";
    if (o->win_first && kmpgpu_set_windows(ctx, o->win_first, o->win_last, o->pats.n)) return "kmpgpu_set_windows";
    _Static_assert(sizeof(kmp_relation) == sizeof(kmpgpu_relation), "kmp_relation has the layout of kmpgpu_relation");
    if (o->relations.n && kmpgpu_set_relations(ctx, (const kmpgpu_relation *)o->relations.rel, o->relations.n)) return "kmpgpu_set_relations";
    _Static_assert(sizeof(kmp_chain_link) == sizeof(kmpgpu_chain_link), "kmp_chain_link has the layout of kmpgpu_chain_link");
    if (o->chains.n && kmpgpu_set_chains(ctx, o->chains.off, (const kmpgpu_chain_link *)o->chains.links, o->chains.n)) return "kmpgpu_set_chains";
    _Static_assert(sizeof(kmp_header) == sizeof(kmpgpu_header) && sizeof(kmp_pkt_meta) == sizeof(kmpgpu_pkt_meta), "kmp_header, kmp_pkt_meta have the layouts of kmpgpu.h");
    if (o->headers.n && kmpgpu_set_headers(ctx, (const kmpgpu_header *)o->headers.hdr, o->headers.n)) return "kmpgpu_set_headers";
    _Static_assert(sizeof(kmp_bytetest) == sizeof(kmpgpu_bytetest), "kmp_bytetest has the layout of kmpgpu_bytetest");
    if (o->bytetests.n && kmpgpu_set_bytetests(ctx, (const kmpgpu_bytetest *)o->bytetests.bt, o->bytetests.n)) return "kmpgpu_set_bytetests";
    if (o->regexes.n && kmpgpu_set_regexes(ctx, o->regexes.expr, o->regexes.len, o->regexes.flags, o->regexes.gate, o->regexes.n)) return "kmpgpu_set_regexes";
    return NULL;
}

static void *shard_load(void *arg)
{
    shard_job *j = (shard_job *)arg;
    const cli_options *o = j->opt;
    if (kmpgpu_init(&j->ctx, j->device)) return shard_fail(j, "kmpgpu_init");
    const char *failed = upload_tables(j->ctx, o);
    if (failed) return shard_fail(j, failed);
    if (o->want_meta && o->device_extract && kmpgpu_set_option(j->ctx, KMPGPU_OPT_KEEP_META, 1)) return shard_fail(j, "kmpgpu_set_option");
    if (o->device_extract) {
        /* only the bytes this shard's frames span are uploaded (kmpgpu_load_frames) */
        const kmp_frames *f = &j->cap->frames;
        if (kmpgpu_load_frames(j->ctx, f->bytes, f->nbytes, f->off + j->lo, f->caplen + j->lo, j->cnt, o->proto == KMP_PROTO_TCP, &j->n_payloads))
            return shard_fail(j, "kmpgpu_load_frames");
    } else {
        const kmp_arena *a = &j->cap->arena;
        const uint64_t hi = j->lo + j->cnt;
        const uint64_t b0 = a->off[j->lo];
        const uint64_t b1 = (hi < a->n_pkts) ? a->off[hi] : a->nbytes;
        j->reb = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)j->cnt);
        if (!j->reb) { j->rc = 1; j->what = "malloc"; snprintf(j->err, sizeof j->err, "out of memory"); return NULL; }
        for (uint64_t k = 0; k < j->cnt; k++) j->reb[k] = a->off[j->lo + k] - b0;
        /* slots are contiguous and at least 16 bytes each, so [b0, b1) holds the whole shard */
        if (kmpgpu_load_arena(j->ctx, a->bytes + b0, b1 - b0, j->reb, a->len + j->lo, j->cnt)) return shard_fail(j, "kmpgpu_load_arena");
        if (j->cap->meta && kmpgpu_set_meta(j->ctx, j->cap->meta + j->lo, j->cnt, 0)) return shard_fail(j, "kmpgpu_set_meta");
    }
    kmpgpu_arena_info(j->ctx, &j->n_payloads, &j->payload_bytes);
    if (kmpgpu_last_timing(j->ctx, &j->t)) return shard_fail(j, "kmpgpu_last_timing");
    return NULL;
}

/* Shards: contiguous ranges of the units, N/P each, the remainder to shard 0 (mpi_dumping.c:149-157); shard r on device
 * r % ndev.  Every shard is brought up by its own host thread -- context, patterns, upload (and extraction) --
 * so that the uploads of the shards run side by side, one PCIe link each (MPI_Scatterv, mpi_dumping.c:161). */
static void start_shards(const cli_options *opt, const capture *cap, uint64_t units, cli_run *run)
{
    const int shards = run->shards;
    shard_job *job = run->job = (shard_job *)calloc((size_t)shards, sizeof *job);
    run->ctxs = (kmpgpu_ctx **)calloc((size_t)shards, sizeof *run->ctxs);
    run->rows = (kmpgpu_ctx **)calloc((size_t)shards, sizeof *run->rows);
    uint64_t lo = 0;
    for (int r = 0; r < shards; r++) {
        job[r].opt = opt; job[r].cap = cap; job[r].device = r % run->ndev;
        job[r].lo = lo; job[r].cnt = units / (uint64_t)shards + (r == 0 ? units % (uint64_t)shards : 0);
        lo += job[r].cnt;
    }
    for (int r = 1; r < shards; r++) {
        job[r].threaded = pthread_create(&job[r].thread, NULL, shard_load, &job[r]) == 0;
        if (!job[r].threaded) shard_load(&job[r]);
    }
    shard_load(&job[0]);
    for (int r = 1; r < shards; r++) if (job[r].threaded) pthread_join(job[r].thread, NULL);
    uint64_t payload_lo = 0;
    for (int r = 0; r < shards; r++) {
        if (job[r].rc) { fprintf(stderr, "%s: %s\n", job[r].what, job[r].err); exit(2); }
        run->ctxs[r] = run->rows[r] = job[r].ctx;
        job[r].payload_lo = payload_lo;
        payload_lo += job[r].n_payloads;
    }
}

/* KMPGPU_OFFSETS_FILE: every match of every shard as a "payload,offset,pattern" line */
static void write_offsets(const char *path, const cli_run *run, uint32_t n_patterns)
{
    FILE *fp = fopen(path, "w");
    if (!fp) { perror("KMPGPU_OFFSETS_FILE"); exit(1); }
    for (int r = 0; r < run->shards; r++) {
        uint64_t total = 0, found = 0;
        for (uint32_t i = 0; i < n_patterns; i++) total += run->own[(size_t)r * n_patterns + i];
        kmpgpu_match *mm = (kmpgpu_match *)malloc(sizeof *mm * (size_t)(total ? total : 1));
        if (!mm || kmpgpu_scan_offsets(run->ctxs[r], mm, total, &found, NULL)) die_gpu("kmpgpu_scan_offsets");
        for (uint64_t i = 0; i < found && i < total; i++)
            fprintf(fp, "%llu,%u,%u\n", (unsigned long long)(mm[i].packet + run->job[r].payload_lo), mm[i].offset, mm[i].pattern);
        free(mm);
    }
    fclose(fp);
}

/* KMPGPU_DECODE: next to every shard a context with the same tables that holds the shard's payloads percent-decoded, every one of them,
 * so that payload numbers stay the capture's; the row outputs come from it. */
static void decode_shards(const cli_options *opt, cli_run *run)
{
    const uint32_t flags = opt->decode == KMP_CLI_DECODE_PLUS ? KMPGPU_DECODE_PLUS : 0u;
    for (int r = 0; r < run->shards; r++) {
        kmpgpu_ctx *d = NULL;
        if (kmpgpu_init(&d, run->job[r].device)) die_gpu("kmpgpu_init");
        const char *failed = upload_tables(d, opt);
        if (failed) die_gpu(failed);
        if (kmpgpu_load_decoded(d, run->ctxs[r], KMPGPU_DECODE_PERCENT, flags, NULL, NULL, NULL)) die_gpu("kmpgpu_load_decoded");
        run->rows[r] = d;
    }
}

/* KMPGPU_BASE64: as decode_shards, the shard's payloads with their base64 runs decoded. */
static void base64_shards(const cli_options *opt, cli_run *run)
{
    const uint32_t flags = opt->base64_url ? KMPGPU_B64_URLSAFE : 0u;
    for (int r = 0; r < run->shards; r++) {
        kmpgpu_ctx *d = NULL;
        if (kmpgpu_init(&d, run->job[r].device)) die_gpu("kmpgpu_init");
        const char *failed = upload_tables(d, opt);
        if (failed) die_gpu(failed);
        if (kmpgpu_load_base64(d, run->ctxs[r], opt->base64_min_run, flags, NULL, NULL, NULL)) die_gpu("kmpgpu_load_base64");
        run->rows[r] = d;
    }
}

/* KMPGPU_HTTP_FIELD: next to every shard a context with the same tables that holds that field of every payload of the shard (an absent
 * field: an empty payload), so that payload numbers stay the capture's; the row outputs come from it.  uri: the raw URI goes through a
 * context of its own, which needs no tables, and its percent-decoding is what is scanned. */
static void field_shards(const cli_options *opt, cli_run *run)
{
    _Static_assert(KMP_CLI_FIELD_METHOD == KMPGPU_FIELD_METHOD && KMP_CLI_FIELD_RAW_URI == KMPGPU_FIELD_RAW_URI && KMP_CLI_FIELD_STATUS == KMPGPU_FIELD_STATUS &&
                   KMP_CLI_FIELD_HEADERS == KMPGPU_FIELD_HEADERS && KMP_CLI_FIELD_BODY == KMPGPU_FIELD_BODY, "KMP_CLI_FIELD_* are the values of KMPGPU_FIELD_*");
    const int uri = opt->http_field == KMP_CLI_FIELD_URI;
    const int field = uri ? KMPGPU_FIELD_RAW_URI : opt->http_field;      /* (KMP_CLI_FIELD_* are the values of KMPGPU_FIELD_*) */
    for (int r = 0; r < run->shards; r++) {
        kmpgpu_ctx *d = NULL, *raw = NULL;
        if (kmpgpu_init(&d, run->job[r].device)) die_gpu("kmpgpu_init");
        const char *failed = upload_tables(d, opt);
        if (failed) die_gpu(failed);
        if (uri) {
            if (kmpgpu_init(&raw, run->job[r].device)) die_gpu("kmpgpu_init");
            if (kmpgpu_load_fields(raw, run->ctxs[r], field, 0u, NULL, NULL, NULL)) die_gpu("kmpgpu_load_fields");
            if (kmpgpu_load_decoded(d, raw, KMPGPU_DECODE_PERCENT, 0u, NULL, NULL, NULL)) die_gpu("kmpgpu_load_decoded");
            kmpgpu_destroy(raw);
        } else if (kmpgpu_load_fields(d, run->ctxs[r], field, 0u, NULL, NULL, NULL)) die_gpu("kmpgpu_load_fields");
        run->rows[r] = d;
    }
}

/* KMPGPU_DNS_FIELD: as field_shards, the dotted name of the first question of every payload of the shard (no message: an empty payload). */
static void dns_shards(const cli_options *opt, cli_run *run)
{
    _Static_assert(KMP_CLI_DNS_QNAME == KMPGPU_DNS_QNAME, "KMP_CLI_DNS_QNAME is the value of KMPGPU_DNS_QNAME");
    const uint32_t flags = opt->dns_tcp ? KMPGPU_DNS_TCP_PREFIX : 0u;
    for (int r = 0; r < run->shards; r++) {
        kmpgpu_ctx *d = NULL;
        if (kmpgpu_init(&d, run->job[r].device)) die_gpu("kmpgpu_init");
        const char *failed = upload_tables(d, opt);
        if (failed) die_gpu(failed);
        if (kmpgpu_load_dns(d, run->ctxs[r], opt->dns_field, flags, NULL, NULL, NULL)) die_gpu("kmpgpu_load_dns");
        run->rows[r] = d;
    }
}

/* KMPGPU_TLS_FIELD: as dns_shards, the server name or the ALPN list of the ClientHello in every payload of the shard (none: an empty
 * payload). */
static void tls_shards(const cli_options *opt, cli_run *run)
{
    _Static_assert(KMP_CLI_TLS_SNI == KMPGPU_TLS_SNI && KMP_CLI_TLS_ALPN == KMPGPU_TLS_ALPN, "KMP_CLI_TLS_* are the values of KMPGPU_TLS_*");
    for (int r = 0; r < run->shards; r++) {
        kmpgpu_ctx *d = NULL;
        if (kmpgpu_init(&d, run->job[r].device)) die_gpu("kmpgpu_init");
        const char *failed = upload_tables(d, opt);
        if (failed) die_gpu(failed);
        if (kmpgpu_load_tls(d, run->ctxs[r], opt->tls_field, 0u, NULL, NULL, NULL)) die_gpu("kmpgpu_load_tls");
        run->rows[r] = d;
    }
}

/* KMPGPU_LINKS_FILE: per shard and distinct buffer a context with the same tables that holds that buffer of every payload of the shard,
 * in the capture's numbering (as decode_shards, base64_shards, field_shards and dns_shards build theirs); on it one single-term rule per
 * link scanned there, whose row kmpgpu_link_rows carries into the shard's own context.  The row outputs stay the shard's own. */
static void links_shards(const cli_options *opt, cli_run *run)
{
    const uint32_t nl = opt->links.n;
    uint32_t *off = (uint32_t *)malloc(sizeof(uint32_t) * ((size_t)nl + 1)), *terms = (uint32_t *)malloc(sizeof(uint32_t) * (nl ? nl : 1)),
             *which = (uint32_t *)malloc(sizeof(uint32_t) * (nl ? nl : 1));
    if (!off || !terms || !which) die_gpu("out of memory");
    for (int r = 0; r < run->shards; r++) {
        if (kmpgpu_set_links(run->ctxs[r], nl)) die_gpu("kmpgpu_set_links");
        for (int b = 0; b < opt->n_link_bufs; b++) {
            const kmp_cli_link_buffer *lb = &opt->link_buf[b];
            kmpgpu_ctx *d = NULL, *raw = NULL;
            if (kmpgpu_init(&d, run->job[r].device)) die_gpu("kmpgpu_init");
            const char *failed = upload_tables(d, opt);
            if (failed) die_gpu(failed);
            if (lb->kind == KMP_CLI_LINK_HTTP && lb->field == KMP_CLI_FIELD_URI) {
                if (kmpgpu_init(&raw, run->job[r].device)) die_gpu("kmpgpu_init");
                if (kmpgpu_load_fields(raw, run->ctxs[r], KMPGPU_FIELD_RAW_URI, 0u, NULL, NULL, NULL)) die_gpu("kmpgpu_load_fields");
                if (kmpgpu_load_decoded(d, raw, KMPGPU_DECODE_PERCENT, 0u, NULL, NULL, NULL)) die_gpu("kmpgpu_load_decoded");
                kmpgpu_destroy(raw);
            } else if (lb->kind == KMP_CLI_LINK_HTTP) {
                if (kmpgpu_load_fields(d, run->ctxs[r], lb->field, 0u, NULL, NULL, NULL)) die_gpu("kmpgpu_load_fields");
            } else if (lb->kind == KMP_CLI_LINK_DNS) {
                if (kmpgpu_load_dns(d, run->ctxs[r], lb->field, lb->flag ? KMPGPU_DNS_TCP_PREFIX : 0u, NULL, NULL, NULL)) die_gpu("kmpgpu_load_dns");
            } else if (lb->kind == KMP_CLI_LINK_DECODE) {
                if (kmpgpu_load_decoded(d, run->ctxs[r], KMPGPU_DECODE_PERCENT, lb->field == KMP_CLI_DECODE_PLUS ? KMPGPU_DECODE_PLUS : 0u, NULL, NULL, NULL))
                    die_gpu("kmpgpu_load_decoded");
            } else if (kmpgpu_load_base64(d, run->ctxs[r], lb->min_run, lb->flag ? KMPGPU_B64_URLSAFE : 0u, NULL, NULL, NULL)) die_gpu("kmpgpu_load_base64");
            /* rule j of d: the term of the j-th link scanned in this buffer */
            uint32_t nr = 0;
            off[0] = 0;
            for (uint32_t q = 0; q < nl; q++)
                if (opt->link_in[q] == b) { terms[nr] = opt->links.term[q]; which[nr] = q; nr++; off[nr] = nr; }
            if (kmpgpu_set_rules(d, off, terms, nr)) die_gpu("kmpgpu_set_rules");
            /* consecutive links of one buffer go in one call: src's pass runs once for them */
            for (uint32_t j = 0; j < nr;) {
                uint32_t k = j + 1;
                while (k < nr && which[k] == which[k - 1] + 1) k++;
                if (kmpgpu_link_rows(run->ctxs[r], which[j], d, KMPGPU_ALERT_RULES, j, k - j, KMPGPU_LINK_SAME, NULL, 0, NULL)) die_gpu("kmpgpu_link_rows");
                j = k;
            }
            kmpgpu_destroy(d);
        }
    }
    free(off); free(terms); free(which);
}

/* The rules on every context the row outputs come from, once: before the first output that needs them (the alerts file, behind its fopen, or the export). */
static void set_rules_once(const cli_options *opt, cli_run *run)
{
    if (run->rules_set || !opt->rules.n) return;
    for (int r = 0; r < run->shards; r++)
        if (kmpgpu_set_rules(run->rows[r], opt->rules.off, opt->rules.terms, opt->rules.n)) die_gpu("kmpgpu_set_rules");
    run->rules_set = 1;
}

/* KMPGPU_FLOWBITS_FILE: the alerts file holds the alert rows of kmpgpu_scan_flowbits instead -- the one shard's payloads grouped into
 * flows, the ops set behind the rules, and one "payload,rule" line per set bit of the rows, by payload, then rule. */
static void write_flowbit_alerts(FILE *fp, const cli_options *opt, cli_run *run)
{
    _Static_assert(sizeof(kmp_flowbit_op) == sizeof(kmpgpu_flowbit_op), "kmp_flowbit_op has the layout of kmpgpu_flowbit_op");
    kmpgpu_ctx *ctx = run->rows[0];
    const uint64_t n = run->job[0].n_payloads, W = (n + 63) / 64, nr = opt->rules.n;
    if (kmpgpu_flows_build(ctx, opt->flows_directed ? KMPGPU_FLOW_DIRECTED : 0u, NULL, NULL)) die_gpu("kmpgpu_flows_build");
    if (kmpgpu_set_flowbits(ctx, (const kmpgpu_flowbit_op *)opt->flowbits.ops, opt->flowbits.n, opt->flowbits.n_bits)) die_gpu("kmpgpu_set_flowbits");
    uint64_t *hits = (uint64_t *)calloc((size_t)(nr * W + 1), sizeof(uint64_t));
    if (!hits) die_gpu("KMPGPU_FLOWBITS_FILE: out of memory");
    if (kmpgpu_scan_flowbits(ctx, NULL, NULL, hits, NULL, NULL, NULL, NULL)) die_gpu("kmpgpu_scan_flowbits");
    for (uint64_t k = 0; k < n; k++)
        for (uint64_t r = 0; r < nr; r++)
            if (hits[r * W + (k >> 6)] >> (k & 63) & 1u) fprintf(fp, "%llu,%llu\n", (unsigned long long)k, (unsigned long long)r);
    free(hits);
}

/* KMPGPU_THRESHOLDS_FILE: the alerts file holds the alert rows of kmpgpu_scan_thresholds instead -- the thresholds set behind the rules,
 * the capture's timestamps, flows only where a by_flow line asks for them, and one "payload,rule" line per set bit, by payload, then rule. */
static void write_threshold_alerts(FILE *fp, const cli_options *opt, cli_run *run)
{
    _Static_assert(sizeof(kmp_threshold) == sizeof(kmpgpu_threshold), "kmp_threshold has the layout of kmpgpu_threshold");
    kmpgpu_ctx *ctx = run->rows[0];
    const uint64_t n = run->job[0].n_payloads, W = (n + 63) / 64, nr = opt->rules.n;
    if (opt->thresholds_by_flow && kmpgpu_flows_build(ctx, opt->flows_directed ? KMPGPU_FLOW_DIRECTED : 0u, NULL, NULL)) die_gpu("kmpgpu_flows_build");
    if (kmpgpu_set_thresholds(ctx, (const kmpgpu_threshold *)opt->thresholds.thr, opt->thresholds.n)) die_gpu("kmpgpu_set_thresholds");
    uint64_t *hits = (uint64_t *)calloc((size_t)(nr * W + 1), sizeof(uint64_t));
    if (!hits) die_gpu("KMPGPU_THRESHOLDS_FILE: out of memory");
    if (kmpgpu_scan_thresholds(ctx, run->job[0].cap->ts, 0, NULL, NULL, hits, NULL, NULL, NULL)) die_gpu("kmpgpu_scan_thresholds");
    for (uint64_t k = 0; k < n; k++)
        for (uint64_t r = 0; r < nr; r++)
            if (hits[r * W + (k >> 6)] >> (k & 63) & 1u) fprintf(fp, "%llu,%llu\n", (unsigned long long)k, (unsigned long long)r);
    free(hits);
}

/* KMPGPU_PACKETS_FILE (family KMPGPU_ALERT_PATTERNS), KMPGPU_ALERTS_FILE (KMPGPU_ALERT_RULES; a rules file without rules leaves the file
 * empty): one "payload,index" line per record of every context's alert list of the family (kmpgpu_scan_alerts: built and sorted by
 * payload, then index, on the device).  The records come back in pieces of a fixed size; no bit matrix leaves the device. */
#define ALERT_PIECE 65536u
static void write_alerts(const char *path, const cli_options *opt, cli_run *run, int family)
{
    static kmpgpu_alert piece[ALERT_PIECE];
    const int by_rules = family == KMPGPU_ALERT_RULES;
    FILE *fp = fopen(path, "w");
    if (!fp) { perror(by_rules ? "KMPGPU_ALERTS_FILE" : "KMPGPU_PACKETS_FILE"); exit(1); }
    if (by_rules) set_rules_once(opt, run);
    if (by_rules && opt->flowbits.n) {
        write_flowbit_alerts(fp, opt, run);
        fclose(fp);
        return;
    }
    if (by_rules && opt->thresholds.n) {
        write_threshold_alerts(fp, opt, run);
        fclose(fp);
        return;
    }
    for (int r = 0; r < (by_rules && !opt->rules.n ? 0 : run->shards); r++) {
        uint64_t found = 0;
        if (kmpgpu_scan_alerts(run->rows[r], family, UINT64_MAX, &found, NULL, NULL, NULL, NULL)) die_gpu("kmpgpu_scan_alerts");
        for (uint64_t first = 0; first < found; first += ALERT_PIECE) {
            const uint64_t n = found - first < ALERT_PIECE ? found - first : ALERT_PIECE;
            if (kmpgpu_alerts_read(run->rows[r], piece, first, n)) die_gpu("kmpgpu_alerts_read");
            for (uint64_t i = 0; i < n; i++) fprintf(fp, "%llu,%u\n", (unsigned long long)(run->job[r].payload_lo + piece[i].packet), piece[i].index);
        }
    }
    fclose(fp);
}

/* KMPGPU_FLOW_STREAMS: next to the shard, whose flows are built, a context with the same tables and rules that holds the shard's flow
 * directions reassembled and groups them into the same n_flows flows; KMPGPU_STREAMS_FILE: its stream records, read back in pieces. */
#define STREAM_PIECE 16384u
static kmpgpu_ctx *stream_context(const cli_options *opt, kmpgpu_ctx *src, const uint32_t *seq, uint64_t n_flows)
{
    static kmpgpu_stream piece[STREAM_PIECE];
    static kmpgpu_stream_order order_piece[STREAM_PIECE];
    const int by_seq = opt->streams_order == KMP_CLI_STREAMS_ORDER_SEQ;
    kmpgpu_ctx *st = NULL;
    uint64_t n_streams = 0, nf = 0;
    if (kmpgpu_init(&st, kmpgpu_device_of(src))) die_gpu("kmpgpu_init");
    const char *failed = upload_tables(st, opt);
    if (failed) die_gpu(failed);
    if (by_seq) {
        /* KMPGPU_FLOW_STREAMS_ORDER=seq: one shard holds every payload, so the capture's sequence numbers are the shard's */
        if (kmpgpu_load_streams_ordered(st, src, opt->flow_streams, seq, 0, &n_streams)) die_gpu("kmpgpu_load_streams_ordered");
    } else if (kmpgpu_load_streams(st, src, opt->flow_streams, &n_streams)) die_gpu("kmpgpu_load_streams");
    if (kmpgpu_flows_build(st, opt->flows_directed ? KMPGPU_FLOW_DIRECTED : 0u, &nf, NULL)) die_gpu("kmpgpu_flows_build");
    if (nf != n_flows) {
        fprintf(stderr, "KMPGPU_FLOW_STREAMS: the streams group into %llu flows, the capture into %llu\n", (unsigned long long)nf, (unsigned long long)n_flows);
        exit(1);
    }
    if (opt->rules.n && kmpgpu_set_rules(st, opt->rules.off, opt->rules.terms, opt->rules.n)) die_gpu("kmpgpu_set_rules");
    if (opt->streams_path) {
        FILE *fp = fopen(opt->streams_path, "w");
        if (!fp) { perror("KMPGPU_STREAMS_FILE"); exit(1); }
        for (uint64_t first = 0; first < n_streams; first += STREAM_PIECE) {
            const uint64_t n = n_streams - first < STREAM_PIECE ? n_streams - first : STREAM_PIECE;
            if (kmpgpu_streams_read(st, piece, first, n)) die_gpu("kmpgpu_streams_read");
            if (by_seq && kmpgpu_stream_orders_read(st, order_piece, first, n)) die_gpu("kmpgpu_stream_orders_read");
            for (uint64_t i = 0; i < n; i++) {
                const kmpgpu_stream *s = &piece[i];
                fprintf(fp, "%llu,%u,%u,%llu,%llu,%llu,%llu,%u", (unsigned long long)(first + i), s->flow, s->dir, (unsigned long long)s->first_packet,
                        (unsigned long long)s->last_packet, (unsigned long long)s->n_packets, (unsigned long long)s->bytes, s->len);
                if (by_seq)
                    fprintf(fp, ",%u,%u,%llu,%llu", order_piece[i].tcp, order_piece[i].n_gaps, (unsigned long long)order_piece[i].gap_bytes,
                            (unsigned long long)order_piece[i].dup_bytes);
                fputc('\n', fp);
            }
        }
        fclose(fp);
    }
    return st;
}

/* KMPGPU_FLOWS_FILE, KMPGPU_FLOW_ALERTS_FILE: the one shard's payloads grouped on the device, the records read back in pieces; then the
 * rules per flow, whose rows come back as a bit matrix of rules x flows (a rules file without rules leaves the file empty). */
#define FLOW_PIECE 16384u
static void write_flows(const cli_options *opt, cli_run *run)
{
    static kmpgpu_flow piece[FLOW_PIECE];
    kmpgpu_ctx *ctx = run->ctxs[0];
    uint64_t n_flows = 0;
    /* the flows file from the payloads as captured (its byte counts are theirs); the flow alerts from the context the rows come from,
     * which groups the same metadata into the same flows */
    if ((opt->flows_path || run->rows[0] == ctx) && kmpgpu_flows_build(ctx, opt->flows_directed ? KMPGPU_FLOW_DIRECTED : 0u, &n_flows, NULL))
        die_gpu("kmpgpu_flows_build");
    if (opt->flows_path) {
        FILE *fp = fopen(opt->flows_path, "w");
        if (!fp) { perror("KMPGPU_FLOWS_FILE"); exit(1); }
        for (uint64_t first = 0; first < n_flows; first += FLOW_PIECE) {
            const uint64_t n = n_flows - first < FLOW_PIECE ? n_flows - first : FLOW_PIECE;
            if (kmpgpu_flows_read(ctx, piece, first, n)) die_gpu("kmpgpu_flows_read");
            for (uint64_t i = 0; i < n; i++) {
                const kmpgpu_flow *f = &piece[i];
                const uint32_t s = f->first.src_ip, d = f->first.dst_ip;
                fprintf(fp, "%llu,%u,%u.%u.%u.%u,%u,%u.%u.%u.%u,%u,%llu,%llu,%llu,%llu\n", (unsigned long long)(first + i), f->first.proto, s >> 24, s >> 16 & 255u,
                        s >> 8 & 255u, s & 255u, f->first.src_port, d >> 24, d >> 16 & 255u, d >> 8 & 255u, d & 255u, f->first.dst_port,
                        (unsigned long long)f->first_packet, (unsigned long long)f->last_packet, (unsigned long long)f->n_packets,
                        (unsigned long long)f->payload_bytes);
            }
        }
        fclose(fp);
    }
    if (opt->flow_alerts_path) {
        FILE *fp = fopen(opt->flow_alerts_path, "w");
        if (!fp) { perror("KMPGPU_FLOW_ALERTS_FILE"); exit(1); }
        if (run->rows[0] != ctx) {
            ctx = run->rows[0];
            if (kmpgpu_flows_build(ctx, opt->flows_directed ? KMPGPU_FLOW_DIRECTED : 0u, &n_flows, NULL)) die_gpu("kmpgpu_flows_build");
        }
        set_rules_once(opt, run);
        const uint64_t Wf = (n_flows + 63) / 64, nr = opt->rules.n;
        kmpgpu_ctx *st = opt->flow_streams ? stream_context(opt, ctx, run->job[0].cap->seq, n_flows) : NULL;
        if (nr && n_flows) {
            uint64_t *hits = (uint64_t *)calloc((size_t)(nr * Wf), sizeof(uint64_t));
            if (!hits) die_gpu("KMPGPU_FLOW_ALERTS_FILE: out of memory");
            if (st) {
                /* KMPGPU_FLOW_STREAMS: the rules per flow over the reassembled streams, whose flows are the capture's */
                if (kmpgpu_scan_flows(st, KMPGPU_ALERT_RULES, KMPGPU_FLOW_SCOPE_FLOW, NULL, NULL, hits, NULL, NULL)) die_gpu("kmpgpu_scan_flows");
            } else if (opt->flow_seams) {
                /* KMPGPU_FLOW_SEAMS: the seams in a context of their own, next to the shard, under the same patterns */
                kmpgpu_ctx *sm = NULL;
                if (kmpgpu_init(&sm, run->job[0].device)) die_gpu("kmpgpu_init");
                if (set_patterns_env(sm, opt->pp, opt->pats.len, opt->pats.n, opt->whole_payload, opt->nocase)) die_gpu("kmpgpu_set_patterns");
                if (kmpgpu_load_seams(sm, ctx, opt->flow_seams, NULL)) die_gpu("kmpgpu_load_seams");
                if (kmpgpu_scan_flows_seams(ctx, sm, NULL, NULL, hits, NULL, NULL)) die_gpu("kmpgpu_scan_flows_seams");
                kmpgpu_destroy(sm);
            } else if (kmpgpu_scan_flows(ctx, KMPGPU_ALERT_RULES, KMPGPU_FLOW_SCOPE_FLOW, NULL, NULL, hits, NULL, NULL)) die_gpu("kmpgpu_scan_flows");
            for (uint64_t f = 0; f < n_flows; f++)
                for (uint64_t r = 0; r < nr; r++)
                    if (hits[r * Wf + (f >> 6)] >> (f & 63) & 1u) fprintf(fp, "%llu,%llu\n", (unsigned long long)f, (unsigned long long)r);
            free(hits);
        }
        if (st) kmpgpu_destroy(st);
        fclose(fp);
    }
}

/* KMPGPU_EXPORT_FILE: the payloads that a rule matches (by_rules) or that hold a pattern, appended shard by shard to the capture that
 * load_options started.  A shard's selection is compacted next to it on its device; only these bytes come back. */
static void write_export(const char *path, const cli_run *run, int by_rules, int have_rules)
{
    uint64_t written = 0;                                                   /* frames in the file so far */
    for (int r = 0; r < run->shards; r++) {
        uint64_t nsel = 0, nb = 0;
        const uint64_t W = (run->job[r].n_payloads + 63) / 64;
        uint64_t *any = (uint64_t *)calloc((size_t)(W ? W : 1), sizeof(uint64_t));
        if (!any) die_gpu("KMPGPU_EXPORT_FILE: out of memory");
        if (by_rules) {                                                     /* (a rules file without rules selects nothing) */
            if (have_rules && kmpgpu_scan_rules(run->ctxs[r], NULL, any, NULL, NULL, NULL)) die_gpu("kmpgpu_scan_rules");
        } else if (kmpgpu_scan_packets(run->ctxs[r], NULL, any, NULL, NULL, NULL)) die_gpu("kmpgpu_scan_packets");
        kmpgpu_ctx *ex = NULL;
        if (kmpgpu_init(&ex, run->job[r].device)) die_gpu("kmpgpu_init");
        if (kmpgpu_load_selected(ex, run->ctxs[r], any, 0, &nsel)) die_gpu("kmpgpu_load_selected");
        free(any);
        if (nsel) {
            if (kmpgpu_arena_download(ex, NULL, 0, &nb, NULL, NULL)) die_gpu("kmpgpu_arena_download");
            uint8_t *bytes = (uint8_t *)malloc((size_t)(nb ? nb : 1));
            uint64_t *off = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)nsel);
            uint32_t *len = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)nsel);
            if (!bytes || !off || !len || kmpgpu_arena_download(ex, bytes, nb, &nb, off, len)) die_gpu("kmpgpu_arena_download");
            if (kmp_write_udp_pcap_part(path, 1, bytes, off, len, nsel, written)) { perror("KMPGPU_EXPORT_FILE"); exit(1); }
            written += nsel;
            free(bytes); free(off); free(len);
        }
        kmpgpu_destroy(ex);
    }
}

/* stderr: what ran where and how fast; with KMPGPU_STATS=1 the text rule, the bytes it bounds and the phases */
static void print_stats(const cli_options *opt, const capture *cap, const cli_run *run, double t_finish)
{
    uint64_t total = 0, h2d_bytes = 0, n_pkts = cap->arena.n_pkts, payload_bytes = cap->arena.payload_bytes;
    double h2d_ms = 0;
    for (uint32_t i = 0; i < opt->pats.n; i++) total += run->counts[i];
    for (int r = 0; r < run->shards; r++) {
        h2d_ms += run->job[r].t.h2d_ms; h2d_bytes += run->job[r].t.h2d_bytes;
        if (opt->device_extract) { n_pkts += run->job[r].n_payloads; payload_bytes += run->job[r].payload_bytes; }      /* (the host arena is empty then) */
    }
    const double bytes = (double)payload_bytes * (double)opt->pats.n;
    fprintf(stderr, "[kmpgpu] %llu frames, %llu payloads, %llu payload bytes, %u patterns, %d shard(s) on %d device(s), count reduce: %s, %llu bytes uploaded\n",
            (unsigned long long)(opt->device_extract ? cap->frames.n : cap->arena.n_frames), (unsigned long long)n_pkts, (unsigned long long)payload_bytes,
            opt->pats.n, run->shards, run->ndev, run->reduce_rccl ? "RCCL all-reduce" : (run->shards > 1 ? "host sum" : "none"), (unsigned long long)h2d_bytes);
    fprintf(stderr, "[kmpgpu] kernel %.3f ms (%.2f GB/s payload x patterns, %.3g matches/s), h2d %.3f ms\n", run->kernel_ms,
            bytes / (run->kernel_ms * 1e6), (double)total / (run->kernel_ms * 1e-3), h2d_ms);
    if (!opt->want_stats) return;
    print_text_rule(opt->whole_payload);
    fprintf(stderr, "[kmpgpu] %llu of the %llu payload bytes lie at or before the first NUL of their payload\n",
            (unsigned long long)run->eff_bytes, (unsigned long long)payload_bytes);
    fprintf(stderr, "[kmpgpu] phases: capture -> host buffers %.3f s, waiting for the HIP runtime %.3f s, contexts + upload + scan %.3f s\n",
            cap->t_loaded - cap->t_load0, cap->t_warm - cap->t_loaded, t_finish - cap->t_warm);
}

int main(int argc, char *argv[])
{
    cli_options opt;
    capture cap;
    cli_run run;
    memset(&run, 0, sizeof run);
    load_options(argc, argv, &opt);
#if !KMP_CLI_OPENMP_FORM
    const double t_start = now_s();                                         /* serial.c:110-111: before the file read */
#endif
    load_capture(&opt, &cap);
#if KMP_CLI_OPENMP_FORM
    const double t_start = now_s();                                         /* openmp_data.c:126: after the pre-load */
#endif
    run.ndev = kmpgpu_device_count();
    if (run.ndev <= 0) die_gpu("no MI355X device");

    const uint32_t n = opt.pats.n;
    const uint64_t units = opt.device_extract ? cap.frames.n : cap.arena.n_pkts;      /* what is split over the shards */
    run.shards = (uint64_t)opt.shards > units ? (int)units : opt.shards;
    run.counts = (uint64_t *)calloc(n ? n : 1, sizeof(uint64_t));
    if (n && units) {
        start_shards(&opt, &cap, units, &run);
        run.own = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)run.shards * n);
        if (!run.own) die_gpu("out of memory");

        run.comm = reduce_comm(run.ctxs, run.shards, run.ndev);
        const double t_scan0 = now_s();
        /* every shard's pass is enqueued before any result is read, so the GPUs work side by side
         * (mpi_dumping.c:198-202: all ranks count, then one reduce) */
        for (int r = 0; r < run.shards; r++)
            if (kmpgpu_scan_enqueue(run.ctxs[r], NULL)) die_gpu("kmpgpu_scan_enqueue");
        run.reduce_rccl = reduce_counts(run.ctxs, run.shards, n, run.own, run.counts, run.comm);
        run.kernel_ms = (now_s() - t_scan0) * 1e3;                          /* wall time of the concurrent passes + reduce (mpi_dumping.c:206 MPI_MAX) */

        if (opt.decode) decode_shards(&opt, &run);
        if (opt.base64_min_run) base64_shards(&opt, &run);
        if (opt.http_field) field_shards(&opt, &run);
        if (opt.dns_field) dns_shards(&opt, &run);
        if (opt.tls_field) tls_shards(&opt, &run);
        if (opt.links.n) links_shards(&opt, &run);
        if (opt.offsets_path) write_offsets(opt.offsets_path, &run, n);
        if (opt.packets_path) write_alerts(opt.packets_path, &opt, &run, KMPGPU_ALERT_PATTERNS);
        if (opt.alerts_path) write_alerts(opt.alerts_path, &opt, &run, KMPGPU_ALERT_RULES);
        if (opt.export_path) {
            set_rules_once(&opt, &run);
            write_export(opt.export_path, &run, opt.rules_path != NULL, opt.rules.n != 0);
        }
        if (opt.flows_path || opt.flow_alerts_path) write_flows(&opt, &run);
        for (int r = 0; r < run.shards && opt.want_stats; r++) {
            uint64_t e = 0;
            if (kmpgpu_effective_bytes(run.ctxs[r], &e)) die_gpu("kmpgpu_effective_bytes");
            run.eff_bytes += e;
        }
    }
    const double t_finish = now_s();                                        /* serial.c:159-160 */

    kmp_report(stdout, &opt.pats, run.counts, t_finish - t_start);         /* serial.c:163-169 */
    /* teardown after the report: serial.c:159-160 takes the time before it frees anything, :178-180 */
    if (run.comm) kmpgpu_comm_destroy(run.comm);
    for (int r = 0; r < run.shards && run.job; r++) {
        if (run.rows[r] != run.ctxs[r]) kmpgpu_destroy(run.rows[r]);
        kmpgpu_destroy(run.ctxs[r]); free(run.job[r].reb);
    }
    if (run.kernel_ms > 0) print_stats(&opt, &cap, &run, t_finish);
    free(run.ctxs); free(run.rows); free(run.job); free(run.own); free(run.counts);
    kmp_arena_free(&cap.arena);
    kmp_frames_free(&cap.frames);
    free(cap.meta);
    free(cap.seq);
    free(cap.ts);
    free_options(&opt);
    return 0;
}
