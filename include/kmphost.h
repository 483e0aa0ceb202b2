/*
 * kmphost.h -- host side of the MI355X KMP packet-payload matcher (plain C, no GPU dependency).
 *
 * These are the pieces of the reference's programs that sit AROUND the hot loop and decide which
 * bytes reach it.  Each entry cites the reference interface it replaces (paths relative to the
 * reference repository).  Library: multithreading_string_matching_amd/lib/libkmphost.so.
 *
 * Conventions: every function returns 0 on success and a negative KMPHOST_E* code on failure;
 * nothing calls exit(); buffers handed in are borrowed, buffers handed out are owned by the
 * struct that carries them and released by its *_free().
 */
#ifndef KMPHOST_H
#define KMPHOST_H

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "kmp_synth.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KMPHOST_OK            0
#define KMPHOST_EIO          -1   /* file cannot be opened / read                       */
#define KMPHOST_EFORMAT      -2   /* not a classic pcap savefile                        */
#define KMPHOST_ENOMEM       -3
#define KMPHOST_EINVAL       -4
#define KMPHOST_ETOKEN       -5   /* pattern token longer than KMP_MAX_PATTERN_LEN      */

#define KMP_MAX_PATTERN_LEN  99   /* serial.c:64  char str[100]                         */
#define KMP_SLOT_ALIGN       16   /* every payload starts on a 16-byte boundary         */
#define KMP_ARENA_SLACK      64   /* readable bytes after the last slot                 */
#define KMP_PROTO_UDP         0   /* serial.c:16                                        */
#define KMP_PROTO_TCP         1   /* serial.c:17                                        */

/* ---- pcap savefile reader ---------------------------------------------------------------
 * Replaces the three libpcap calls the reference makes: pcap_open_offline (serial.c:91,
 * openmp_data.c:94), pcap_next_ex (serial.c:115, openmp_data.c:107), pcap_close.  Classic pcap
 * (magic a1b2c3d4 / a1b23c4d, either byte order) and pcapng (enhanced, simple and obsolete packet
 * blocks, either byte order, several sections) -- the two formats libpcap's pcap_open_offline reads;
 * libpcap itself is not in this image. */
typedef struct kmp_pcap kmp_pcap;
#define KMP_PCAP_ERRBUF 256                       /* PCAP_ERRBUF_SIZE analogue, serial.c:26 */
kmp_pcap *kmp_pcap_open(const char *path, char errbuf[KMP_PCAP_ERRBUF]);
/* 1 = packet returned (data valid until the next call), -2 = end of file, -1 = truncated record;
 * the reference's loop ends on either negative value (serial.c:115). */
int  kmp_pcap_next(kmp_pcap *p, uint32_t *caplen, uint32_t *len, const uint8_t **data);
uint32_t kmp_pcap_linktype(const kmp_pcap *p);
void kmp_pcap_close(kmp_pcap *p);

/* ---- payload extraction -------------------------------------------------------------------
 * Replace dump_UDP_packet (packet_dumping.h:87-139) and dump_TCP_packet (packet_dumping.h:150-188):
 * return 1 and the payload's offset/length inside the frame, or 0 where the reference returns
 * NULL.  Quirks kept: no EtherType / IP-version test, IHL from the low nibble of frame byte 14,
 * UDP header skipped as 8 bytes, payload = all remaining captured bytes.  The
 * TCP variant additionally rejects frames on which the reference's unsigned length would wrap. */
int kmp_extract_udp(const uint8_t *frame, uint32_t capture_len, uint32_t *payload_off, uint32_t *payload_len);
int kmp_extract_tcp(const uint8_t *frame, uint32_t capture_len, uint32_t *payload_off, uint32_t *payload_len);

/* The header fields the extractors walk past on their way to the payload (kmpgpu_pkt_meta of include/kmpgpu.h has this layout): with p the
 * frame, src_ip = p[26]<<24 | p[27]<<16 | p[28]<<8 | p[29] and dst_ip from p[30..33] (host-order integers), the ports from
 * T = 14 + ((p[14] & 0x0F) << 2) as p[T]<<8 | p[T+1] and p[T+2]<<8 | p[T+3], proto = p[23].  The byte positions are the extractors' own,
 * quirks included: no EtherType or IP-version test, and in tcp mode nothing has tested p[23].  kmp_extract_meta returns 1 / 0 exactly
 * where kmp_extract_udp (proto == KMP_PROTO_UDP) / kmp_extract_tcp (KMP_PROTO_TCP) do; for an accepted frame every byte read lies
 * inside capture_len, for a rejected one *out is not written. */
typedef struct kmp_pkt_meta {
    uint32_t src_ip, dst_ip;
    uint16_t src_port, dst_port;
    uint8_t  proto;
    uint8_t  reserved[3];     /* 0 */
} kmp_pkt_meta;
int kmp_extract_meta(const uint8_t *frame, uint32_t capture_len, int proto, kmp_pkt_meta *out);
/* The TCP sequence number (kmpgpu_load_streams_ordered takes one per payload): the big-endian 32 bits at T + 4.  Returns 1 / 0 exactly
 * where the extractor of `proto` does; for an accepted frame those bytes lie inside capture_len (for a UDP frame they are its length and
 * checksum, and no stream of UDP payloads looks at them), for a rejected one *seq is not written. */
int kmp_extract_tcp_seq(const uint8_t *frame, uint32_t capture_len, int proto, uint32_t *seq);

/* ---- pattern list -------------------------------------------------------------------------
 * Replaces the fscanf("%s") loader of serial.c:54-87 / openmp_data.c:57-90: whitespace-separated
 * tokens in file order, duplicates kept. */
typedef struct kmp_patterns {
    uint32_t  n;          /* number of tokens                              */
    uint8_t  *blob;       /* all tokens back to back, each NUL-terminated  */
    uint32_t *off;        /* off[i]: start of token i in blob              */
    uint32_t *len;        /* len[i]: strlen of token i (1..99)             */
} kmp_patterns;
int  kmp_patterns_load(const char *path, kmp_patterns *out);                 /* KMPHOST_EIO: errno is set, as for fopen (serial.c:59-63) */
int  kmp_patterns_parse(const uint8_t *text, size_t n, kmp_patterns *out);
void kmp_patterns_free(kmp_patterns *p);

/* ---- content rules --------------------------------------------------------------------------
 * Not in the reference: the rules of kmpgpu_set_rules (include/kmpgpu.h) from a text file.  One rule per line; its terms are
 * separated by blanks; a term is a decimal pattern index (the position in the pattern file, 0-based) with an optional leading '!'
 * for a pattern that must NOT be in the payload.  Blank lines and lines whose first non-blank character is '#' are skipped; rule
 * index = order of the rule lines.  off / terms are what kmpgpu_set_rules takes: rule r = terms[off[r] .. off[r + 1]), a negated
 * term carries KMP_RULE_NOT (= KMPGPU_RULE_NOT).
 * KMPHOST_EIO: the file cannot be opened; KMPHOST_EINVAL: a term that is not a number, an index >= n_patterns, a bare '!' --
 * errbuf then starts with "line N: " (N counts every line of the file, from 1). */
#define KMP_RULE_NOT      0x80000000u
#define KMP_RULES_ERRBUF  256
typedef struct kmp_rules {
    uint32_t  n;          /* number of rules                               */
    uint32_t *off;        /* [n + 1]                                       */
    uint32_t *terms;      /* [off[n]]                                      */
} kmp_rules;
int  kmp_rules_parse(const char *path, uint32_t n_patterns, kmp_rules *out, char errbuf[KMP_RULES_ERRBUF]);
/* The same with relations as terms (kmpgpu_set_relations): "r<q>" / "!r<q>", q < n_relations a decimal relation index (the order of
 * the relation lines of kmp_relations_parse), is encoded as n_patterns + q, the row kmpgpu_set_rules knows it by.  A relation index
 * >= n_relations: KMPHOST_EINVAL, "line N: ".  n_patterns + n_relations >= 2^31 (a term's bit 31 is KMP_RULE_NOT): KMPHOST_EINVAL
 * before the file is opened, errbuf without a line number.  kmp_rules_parse is this with n_relations = 0, where "r3" is no term at all. */
int  kmp_rules_parse_rel(const char *path, uint32_t n_patterns, uint32_t n_relations, kmp_rules *out, char errbuf[KMP_RULES_ERRBUF]);
/* ... and with chains as terms (kmpgpu_set_chains): "c<q>" / "!c<q>", q < n_chains a decimal chain index (the order of the chain lines of
 * kmp_chains_parse), is encoded as n_patterns + n_relations + q.  A chain index >= n_chains: KMPHOST_EINVAL, "line N: ".
 * n_patterns + n_relations + n_chains >= 2^31: KMPHOST_EINVAL before the file is opened.  kmp_rules_parse_rel is this with n_chains = 0,
 * where "c3" is no term at all. */
int  kmp_rules_parse_terms(const char *path, uint32_t n_patterns, uint32_t n_relations, uint32_t n_chains, kmp_rules *out,
                           char errbuf[KMP_RULES_ERRBUF]);
/* ... and with header predicates as terms (kmpgpu_set_headers): "h<q>" / "!h<q>", q < n_headers a decimal predicate index (the order of the
 * lines of kmp_headers_parse), is encoded as n_patterns + n_relations + n_chains + q.  A predicate index >= n_headers: KMPHOST_EINVAL,
 * "line N: ".  n_patterns + n_relations + n_chains + n_headers >= 2^31: KMPHOST_EINVAL before the file is opened.  kmp_rules_parse_terms
 * is this with n_headers = 0, where "h3" is no term at all. */
int  kmp_rules_parse_hdr(const char *path, uint32_t n_patterns, uint32_t n_relations, uint32_t n_chains, uint32_t n_headers, kmp_rules *out,
                         char errbuf[KMP_RULES_ERRBUF]);
/* ... and with byte tests as terms (kmpgpu_set_bytetests): "b<q>" / "!b<q>", q < n_bytetests a decimal test index (the order of the lines of
 * kmp_bytetests_parse), is encoded as n_patterns + n_relations + n_chains + n_headers + q.  A test index >= n_bytetests: KMPHOST_EINVAL,
 * "line N: ".  n_patterns + n_relations + n_chains + n_headers + n_bytetests >= 2^31: KMPHOST_EINVAL before the file is opened.
 * kmp_rules_parse_hdr is this with n_bytetests = 0, where "b3" is no term at all and every message is what it was. */
int  kmp_rules_parse_bt(const char *path, uint32_t n_patterns, uint32_t n_relations, uint32_t n_chains, uint32_t n_headers, uint32_t n_bytetests,
                        kmp_rules *out, char errbuf[KMP_RULES_ERRBUF]);
/* ... and with expressions as terms (kmpgpu_set_regexes): "x<q>" / "!x<q>", q < n_regexes a decimal expression index (the order of the lines
 * of kmp_regexes_parse), is encoded as n_patterns + n_relations + n_chains + n_headers + n_bytetests + q.  An expression index >= n_regexes:
 * KMPHOST_EINVAL, "line N: ".  n_patterns + n_relations + n_chains + n_headers + n_bytetests + n_regexes >= 2^31: KMPHOST_EINVAL before the
 * file is opened.  kmp_rules_parse_bt is this with n_regexes = 0, where "x3" is no term at all and every message is what it was. */
int  kmp_rules_parse_rx(const char *path, uint32_t n_patterns, uint32_t n_relations, uint32_t n_chains, uint32_t n_headers, uint32_t n_bytetests,
                        uint32_t n_regexes, kmp_rules *out, char errbuf[KMP_RULES_ERRBUF]);
/* The same once more with the links of kmpgpu_set_links behind the expressions: "l<q>" / "!l<q>" is link q, row
 * n_patterns + ... + n_regexes + q.  Without links (n_links = 0) the token is no term at all, as with the other letters. */
int  kmp_rules_parse_links(const char *path, uint32_t n_patterns, uint32_t n_relations, uint32_t n_chains, uint32_t n_headers,
                           uint32_t n_bytetests, uint32_t n_regexes, uint32_t n_links, kmp_rules *out, char errbuf[KMP_RULES_ERRBUF]);
void kmp_rules_free(kmp_rules *r);

/* ---- links -----------------------------------------------------------------------------------
 * Not in the reference: the links file of the programs (KMPGPU_LINKS_FILE).  One link per line,
 *     <buffer> <term>
 * link q (the q-th such line) is the row <term> -- ONE un-negated token of the rules syntax over the shared tables ("7", "r0", "c1",
 * "h0", "b0", "x2") -- scanned in the buffer <buffer>, a word of at most KMP_LINK_BUFFER - 1 characters that the caller interprets
 * ("http:body", "dns:qname,tcp", "decode:percent", "base64:16,url").  Blank lines and lines that start with '#' are skipped.  A negated
 * term, an l<q> term (a link names no link), a term out of range, a second term, a line without a term or a buffer word that is too
 * long: KMPHOST_EINVAL with "line N: ..." in errbuf. */
#define KMP_LINKS_ERRBUF 256
#define KMP_LINK_BUFFER 64
typedef struct kmp_links {
    uint32_t  n;                          /* number of links                                  */
    char    (*buffer)[KMP_LINK_BUFFER];   /* [n]: the buffer word, NUL-terminated             */
    uint32_t *term;                       /* [n]: the row the link's single-term rule names   */
} kmp_links;
int  kmp_links_parse(const char *path, uint32_t n_patterns, uint32_t n_relations, uint32_t n_chains, uint32_t n_headers, uint32_t n_bytetests,
                     uint32_t n_regexes, kmp_links *out, char errbuf[KMP_LINKS_ERRBUF]);
void kmp_links_free(kmp_links *l);

/* ---- relations -------------------------------------------------------------------------------
 * Not in the reference: the relations of kmpgpu_set_relations (include/kmpgpu.h) from a text file.  One relation per line,
 *     <a> <b> <dmin> <dmax>
 * four fields separated by blanks: two pattern indices (positions in the pattern file, 0-based) and the bounds on
 * (start of b) - (end of a), decimal and possibly negative; '*' for <dmin> means no lower bound (INT32_MIN), for <dmax> no upper
 * bound (INT32_MAX).  Blank lines and lines whose first non-blank character is '#' are skipped; relation index = order of the
 * relation lines.  rel is what kmpgpu_set_relations takes (kmp_relation has the layout of kmpgpu_relation).
 * KMPHOST_EIO: the file cannot be opened; KMPHOST_EINVAL: a field that is not a number (or does not fit 32 bits), a line of fewer or
 * more than four fields, an index >= n_patterns, dmin > dmax -- errbuf then starts with "line N: " (N counts every line of the
 * file, from 1). */
#define KMP_RELATIONS_ERRBUF 256
typedef struct kmp_relation { uint32_t a, b; int32_t dmin, dmax; } kmp_relation;
typedef struct kmp_relations {
    uint32_t      n;      /* number of relations                           */
    kmp_relation *rel;    /* [n]                                           */
} kmp_relations;
int  kmp_relations_parse(const char *path, uint32_t n_patterns, kmp_relations *out, char errbuf[KMP_RELATIONS_ERRBUF]);
void kmp_relations_free(kmp_relations *r);

/* ---- chains ----------------------------------------------------------------------------------
 * Not in the reference: the chains of kmpgpu_set_chains (include/kmpgpu.h) from a text file.  One chain per line,
 *     <p0> <dmin> <dmax> <p1> [<dmin> <dmax> <p2> ...]
 * 3n - 2 fields separated by blanks for a chain of n contents, 2 <= n <= KMP_CHAIN_MAX: pattern indices (positions in the pattern file,
 * 0-based) with, between two of them, the bounds on (start of the next content) - (end of the one before), decimal and possibly
 * negative; '*' for <dmin> means no lower bound (INT32_MIN), for <dmax> no upper bound (INT32_MAX).  Blank lines and lines whose first
 * non-blank character is '#' are skipped; chain index = order of the chain lines.  off / links are what kmpgpu_set_chains takes
 * (kmp_chain_link has the layout of kmpgpu_chain_link; a chain's first link carries INT32_MIN / INT32_MAX).
 * KMPHOST_EIO: the file cannot be opened; KMPHOST_EINVAL: a field that is not a number (or does not fit 32 bits), a field count that is
 * not 3n - 2, fewer than 2 or more than KMP_CHAIN_MAX contents, an index >= n_patterns, dmin > dmax -- errbuf then starts with
 * "line N: " (N counts every line of the file, from 1). */
#define KMP_CHAINS_ERRBUF 256
#define KMP_CHAIN_MAX     8
typedef struct kmp_chain_link { uint32_t pattern; int32_t dmin, dmax; } kmp_chain_link;
typedef struct kmp_chains {
    uint32_t        n;      /* number of chains                              */
    uint32_t       *off;    /* [n + 1]                                       */
    kmp_chain_link *links;  /* [off[n]]                                      */
} kmp_chains;
int  kmp_chains_parse(const char *path, uint32_t n_patterns, kmp_chains *out, char errbuf[KMP_CHAINS_ERRBUF]);
void kmp_chains_free(kmp_chains *c);

/* ---- header predicates -----------------------------------------------------------------------
 * Not in the reference: the predicates of kmpgpu_set_headers (include/kmpgpu.h) from a text file.  One predicate per line,
 *     <proto> <src> <sport> <dir> <dst> <dport> [<len>]
 * six or seven fields separated by blanks.  <proto>: udp (17), tcp (6), ip or any (KMP_HDR_ANY_PROTO), or decimal 0..255.  <src>, <dst>:
 * any (mask 0), a.b.c.d (mask /32) or a.b.c.d/n with n = 0..32.  <sport>, <dport> (0..65535) and <len> (0..4294967295, on the payload's
 * length; absent: any): any, n, lo:hi, lo: or :hi.  <dir>: -> or <> (KMP_HDR_BIDIR: the predicate also holds with source and destination
 * swapped).  Blank lines and lines whose first non-blank character is '#' are skipped; predicate index = order of the lines.  hdr is
 * what kmpgpu_set_headers takes (kmp_header has the layout of kmpgpu_header).
 * KMPHOST_EIO: the file cannot be opened; KMPHOST_EINVAL: fewer than six or more than seven fields, a field of none of its forms, a
 * number out of its range, lo > hi -- errbuf then starts with "line N: " (N counts every line of the file, from 1). */
#define KMP_HEADERS_ERRBUF 256
#define KMP_HDR_ANY_PROTO  1u
#define KMP_HDR_BIDIR      2u
typedef struct kmp_header {
    uint32_t src_ip, src_mask, dst_ip, dst_mask;
    uint16_t sport_lo, sport_hi, dport_lo, dport_hi;
    uint32_t len_lo, len_hi;
    uint8_t  proto, flags;
    uint16_t reserved;        /* 0 */
} kmp_header;
typedef struct kmp_headers {
    uint32_t    n;      /* number of predicates                          */
    kmp_header *hdr;    /* [n]                                           */
} kmp_headers;
int  kmp_headers_parse(const char *path, kmp_headers *out, char errbuf[KMP_HEADERS_ERRBUF]);
void kmp_headers_free(kmp_headers *h);

/* ---- byte tests ------------------------------------------------------------------------------
 * Not in the reference: the tests of kmpgpu_set_bytetests (include/kmpgpu.h) from a text file.  One test per line,
 *     <nbytes> <op> <value> <offset> [after <pattern index>] [little] [mask <m>]
 * fields separated by blanks: read <nbytes> (1..4) bytes at <offset>, take them as a big-endian integer (little: little-endian), AND
 * them with <m> (absent: all bits) and compare with <value> by <op>, one of = != < > <= >= &.  "&" is the bit test: it sets
 * mask = <value> and asks for a result other than 0 (KMP_BT_NE against 0), and refuses a mask clause.  after <i> makes the test relative:
 * <offset>, then of any sign, counts from the end of a match of pattern i (a position in the pattern file, 0-based); without it <offset>
 * counts from the payload's first byte and is not negative.  Numbers are decimal or 0x hex; the three clauses come in any order, each at
 * most once.  Blank lines and lines whose first non-blank character is '#' are skipped; test index = order of the lines.  bt is what
 * kmpgpu_set_bytetests takes (kmp_bytetest has the layout of kmpgpu_bytetest).
 * KMPHOST_EIO: the file cannot be opened; KMPHOST_EINVAL: fewer than four fields, a field of none of its forms, a number out of its
 * range, an index >= n_patterns, an unknown or repeated clause, a negative offset without after -- errbuf then starts with "line N: "
 * (N counts every line of the file, from 1). */
#define KMP_BYTETESTS_ERRBUF 256
#define KMP_BT_RELATIVE    1u
#define KMP_BT_LITTLE      2u
enum { KMP_BT_EQ, KMP_BT_NE, KMP_BT_LT, KMP_BT_GT, KMP_BT_LE, KMP_BT_GE };
typedef struct kmp_bytetest {
    uint32_t anchor;
    int32_t  offset;
    uint32_t mask, value;
    uint8_t  nbytes, op, flags, reserved;   /* reserved: 0 */
} kmp_bytetest;
typedef struct kmp_bytetests {
    uint32_t      n;      /* number of tests                               */
    kmp_bytetest *bt;     /* [n]                                           */
} kmp_bytetests;
int  kmp_bytetests_parse(const char *path, uint32_t n_patterns, kmp_bytetests *out, char errbuf[KMP_BYTETESTS_ERRBUF]);
void kmp_bytetests_free(kmp_bytetests *b);

/* ---- expressions -----------------------------------------------------------------------------
 * Not in the reference: the expressions of kmpgpu_set_regexes (include/kmpgpu.h, where the dialect is) from a text file.  One per line,
 *     /EXPR/[i][s] [with <pattern index>]
 * EXPR runs from behind the first '/' to the last '/' of the line and is taken byte for byte (a '/' inside it needs no escape); i makes it
 * case-insensitive (KMP_RX_NOCASE), s lets the dot match a newline (KMP_RX_DOTALL), a third letter e ("extended", KMP_RX_GROUPS) makes
 * ( ), (?: ) and | groups and alternation: /(GET|POST) \//ie with 3; with <i> gates it on pattern i (a position in the
 * pattern file, 0-based; KMP_RX_GATED): it is looked at only in payloads that hold that pattern.  Blank lines and lines whose first
 * non-blank character is '#' are skipped; expression index = order of the lines.  expr, len, flags and gate are what kmpgpu_set_regexes
 * takes; the dialect itself is checked there, not here.
 * KMPHOST_EIO: the file cannot be opened; KMPHOST_EINVAL: a line that does not start with '/', no closing '/', an empty expression, an
 * unknown or repeated flag, anything but with <pattern index> behind the flags, an index >= n_patterns -- errbuf then starts with
 * "line N: " (N counts every line of the file, from 1). */
#define KMP_REGEXES_ERRBUF 256
#define KMP_RX_NOCASE 1u
#define KMP_RX_DOTALL 2u
#define KMP_RX_GATED  4u
#define KMP_RX_GROUPS 16u     /* flag letter e ("extended"): groups and alternation (KMPGPU_RX_GROUPS), /(GET|POST) \//ie with 3 */
typedef struct kmp_regexes {
    uint32_t        n;       /* number of expressions                                  */
    const uint8_t **expr;    /* [n]: expression q, len[q] bytes, inside `bytes`         */
    uint32_t       *len;     /* [n]                                                    */
    uint32_t       *flags;   /* [n]: KMP_RX_*                                          */
    uint32_t       *gate;    /* [n]: the gate pattern with KMP_RX_GATED, else 0        */
    uint8_t        *bytes;   /* the expressions back to back                           */
    uint32_t       *off;     /* [n + 1]: where each starts in `bytes`                  */
} kmp_regexes;
int  kmp_regexes_parse(const char *path, uint32_t n_patterns, kmp_regexes *out, char errbuf[KMP_REGEXES_ERRBUF]);
void kmp_regexes_free(kmp_regexes *r);

/* ---- flow bits -------------------------------------------------------------------------------
 * Not in the reference: the ops of kmpgpu_set_flowbits (include/kmpgpu.h, where they are defined) from a text file.  One line
 *     <rule> <word> [<word> ...]
 * gives rule <rule> (a decimal position in the rules file, 0-based) the words' tests and actions in their order: set:<name>
 * unset:<name> toggle:<name> isset:<name> isnotset:<name> and noalert.  A name is 1..31 characters of [A-Za-z0-9_.-]; names are numbered
 * by first appearance, at most KMP_FLOWBITS_MAX of them.  A rule may have several lines.  Blank lines and lines whose first non-blank
 * character is '#' are skipped.  ops is what kmpgpu_set_flowbits takes (kmp_flowbit_op has the layout of kmpgpu_flowbit_op), n_bits the
 * number of names (1 where only noalert was used); names[b] is bit b's.
 * KMPHOST_EIO: the file cannot be opened; KMPHOST_EINVAL: a rule that is no number below n_rules, a line without a word, an unknown word,
 * a name of none of its forms, a 33rd name, a (rule, name) tested both ways -- errbuf then starts with "line N: " (N counts every line of
 * the file, from 1) --, and, found when the file has been read, names that form a cycle (a rule tests one and acts on the next):
 * errbuf names them in the cycle's order. */
#define KMP_FLOWBITS_ERRBUF 256
#define KMP_FLOWBITS_MAX    32
#define KMP_FLOWBIT_NAME    32     /* bytes of a name with its 0x00 */
enum { KMP_FB_ISSET, KMP_FB_ISNOTSET, KMP_FB_SET, KMP_FB_UNSET, KMP_FB_TOGGLE, KMP_FB_NOALERT };
typedef struct kmp_flowbit_op { uint32_t rule, bit, op, reserved; } kmp_flowbit_op;
typedef struct kmp_flowbits {
    uint32_t        n, n_bits;      /* number of ops; of names                       */
    kmp_flowbit_op *ops;            /* [n]                                           */
    char            names[KMP_FLOWBITS_MAX][KMP_FLOWBIT_NAME];
} kmp_flowbits;
int  kmp_flowbits_parse(const char *path, uint32_t n_rules, kmp_flowbits *out, char errbuf[KMP_FLOWBITS_ERRBUF]);
void kmp_flowbits_free(kmp_flowbits *f);

/* ---- rate thresholds -------------------------------------------------------------------------
 * Not in the reference: the thresholds of kmpgpu_set_thresholds (include/kmpgpu.h, where they are defined) from a text file.  One line
 *     <rule> by_rule|by_src|by_dst|by_flow at_least|at_most|exactly <count> <seconds|all>
 * gives rule <rule> (a decimal position in the rules file, 0-based) one threshold; a rule may have several lines.  <count> is 1..2^32 - 1.
 * <seconds> is decimal with at most 6 fraction digits (60, 0.5) and is converted exactly to microseconds, the unit of
 * kmp_arena_from_pcap_ts; `all` is KMP_THR_NO_WINDOW.  Blank lines and lines whose first non-blank character is '#' are skipped.  thr is
 * what kmpgpu_set_thresholds takes (kmp_threshold has the layout of kmpgpu_threshold).
 * KMPHOST_EIO: the file cannot be opened; KMPHOST_EINVAL: a rule that is no number below n_rules, a missing field, an unknown track or
 * type, a count that is no number in its range, a window that is neither `all` nor such seconds, that is 0, or that is more than
 * 2^64 - 2 microseconds, a field behind the window -- errbuf names the line (a position in the file, from 1). */
#define KMP_THRESHOLDS_ERRBUF 256
#define KMP_THR_NO_WINDOW     (~0ull)
enum { KMP_THR_BY_RULE, KMP_THR_BY_SRC, KMP_THR_BY_DST, KMP_THR_BY_FLOW };
enum { KMP_THR_AT_LEAST, KMP_THR_AT_MOST, KMP_THR_EXACTLY };
typedef struct kmp_threshold { uint32_t rule, track, type, count; uint64_t window; } kmp_threshold;
typedef struct kmp_thresholds {
    uint32_t       n;               /* number of thresholds                          */
    kmp_threshold *thr;             /* [n]                                           */
} kmp_thresholds;
int  kmp_thresholds_parse(const char *path, uint32_t n_rules, kmp_thresholds *out, char errbuf[KMP_THRESHOLDS_ERRBUF]);
void kmp_thresholds_free(kmp_thresholds *t);

/* ---- offset windows --------------------------------------------------------------------------
 * Not in the reference: the windows of kmpgpu_set_windows (include/kmpgpu.h) from a text file.  One window per line,
 *     <pattern index> <first> <last>
 * three decimal fields separated by blanks: the pattern's position in the pattern file (0-based) and the first and the last start
 * offset inside a payload at which a match of it is reported; '*' for <last> means no upper bound (UINT32_MAX).  Blank lines and
 * lines whose first non-blank character is '#' are skipped; a pattern that no line names keeps the default window [0, UINT32_MAX].
 * first_out / last_out have room for n_patterns values each and are what kmpgpu_set_windows takes; on an error their contents are
 * unspecified.
 * KMPHOST_EIO: the file cannot be opened; KMPHOST_EINVAL: a field that is not a number (or does not fit 32 bits), a line of fewer
 * or more than three fields, an index >= n_patterns, first > last, a pattern named twice -- errbuf then starts with "line N: "
 * (N counts every line of the file, from 1). */
#define KMP_WINDOWS_ERRBUF 256
int  kmp_windows_parse(const char *path, uint32_t n_patterns, uint32_t *first_out, uint32_t *last_out, char errbuf[KMP_WINDOWS_ERRBUF]);

/* KMP failure function: replaces kmp_prefix (serial.c:217-238); prefix has room for m ints. */
void kmp_failure_table(const uint8_t *pat, uint32_t m, int32_t *prefix);

/* ---- payload arena -------------------------------------------------------------------------
 * Replaces char **array_of_payloads (serial.c:99,124-136; openmp_data.c:123,139-142): one
 * contiguous byte arena, payload k at bytes[off[k] .. off[k]+len[k]), off[k] % 16 == 0, the gap
 * up to the next slot zero-filled, KMP_ARENA_SLACK readable zero bytes after the last slot.
 * Memory comes from the allocator pair so the caller can make it pinned (kmpgpu_host_alloc). */
typedef void *(*kmp_alloc_fn)(size_t);
typedef void  (*kmp_free_fn)(void *);
typedef struct kmp_arena {
    uint8_t  *bytes;
    uint64_t  nbytes;         /* allocated size of bytes, slack included                */
    uint64_t *off;
    uint32_t *len;
    uint64_t  n_pkts;         /* payloads stored (invalid frames are skipped, serial.c:138-140) */
    uint64_t  payload_bytes;  /* sum of len[]                                            */
    uint64_t  n_frames;       /* records read from the savefile                          */
    kmp_free_fn free_fn;
} kmp_arena;
/* serial.c:115-141: read every record, extract, store.  capture length handed to the extractor is
 * caplen (openmp_data.c:116,131; equals serial.c's header->len whenever caplen == len). */
int  kmp_arena_from_pcap(const char *path, int proto, kmp_alloc_fn alloc_fn, kmp_free_fn free_fn,
                         kmp_arena *out, char errbuf[KMP_PCAP_ERRBUF]);
/* The identical arena, and beside it the accepted frames' header fields in payload order (kmp_extract_meta): *meta_out holds
 * out->n_pkts records, comes from malloc() and is released with free().  kmp_arena's layout is the same either way. */
int  kmp_arena_from_pcap_meta(const char *path, int proto, kmp_alloc_fn alloc_fn, kmp_free_fn free_fn,
                              kmp_arena *out, char errbuf[KMP_PCAP_ERRBUF], kmp_pkt_meta **meta_out);
/* ... and beside both the accepted frames' sequence numbers in payload order (kmp_extract_tcp_seq): *seq_out holds out->n_pkts words,
 * comes from malloc() and is released with free().  meta_out and seq_out may each be NULL. */
int  kmp_arena_from_pcap_seq(const char *path, int proto, kmp_alloc_fn alloc_fn, kmp_free_fn free_fn,
                             kmp_arena *out, char errbuf[KMP_PCAP_ERRBUF], kmp_pkt_meta **meta_out, uint32_t **seq_out);
/* The arena and the metadata of kmp_arena_from_pcap_meta, and beside them the accepted frames' capture times in payload order, in
 * microseconds, as kmpgpu_scan_thresholds takes them: *ts_out holds out->n_pkts words, comes from malloc() and is released with free().
 * Classic pcap: ts_sec * 1e6 + ts_frac; under the nanosecond magic 0xA1B23C4D ts_sec * 1e6 + ts_frac / 1000.  pcapng: the block's 64-bit
 * timestamp taken as microseconds (if_tsresol is not parsed; a Simple Packet Block has none: 0).  meta_out and ts_out may each be NULL.
 * kmp_arena_from_pcap_seq_ts: the same with seq_out as kmp_arena_from_pcap_seq gives it; every out array may be NULL. */
int  kmp_arena_from_pcap_ts(const char *path, int proto, kmp_alloc_fn alloc_fn, kmp_free_fn free_fn,
                            kmp_arena *out, char errbuf[KMP_PCAP_ERRBUF], kmp_pkt_meta **meta_out, uint64_t **ts_out);
int  kmp_arena_from_pcap_seq_ts(const char *path, int proto, kmp_alloc_fn alloc_fn, kmp_free_fn free_fn,
                                kmp_arena *out, char errbuf[KMP_PCAP_ERRBUF], kmp_pkt_meta **meta_out, uint32_t **seq_out, uint64_t **ts_out);
/* Build an arena from caller-supplied payloads (tests, synthetic inputs). */
int  kmp_arena_from_payloads(const uint8_t *const *payloads, const uint32_t *lens, uint64_t n,
                             kmp_alloc_fn alloc_fn, kmp_free_fn free_fn, kmp_arena *out);
/* Index for n fixed-length payloads / for given lengths; returns the arena size needed. */
uint64_t kmp_arena_layout(const uint32_t *lens, uint32_t fixed_len, uint64_t n, uint32_t slot_align,
                          uint64_t *off_out, uint32_t *len_out);
void kmp_arena_free(kmp_arena *a);

/* ---- raw frames for on-device extraction ------------------------------------------------------
 * The capture file as it is + where its frames lie: everything the host does when the payload
 * extraction (openmp_data.c:128-147) runs on the GPU (kmpgpu_load_frames).  Walking the record
 * headers is the only sequential part of a pcap file. */
typedef struct kmp_frames {
    uint8_t  *bytes;          /* the whole savefile                                  */
    uint64_t  nbytes;
    uint64_t *off;            /* off[f]: first byte of frame f inside bytes          */
    uint32_t *caplen;         /* caplen[f]: captured bytes of frame f                */
    uint64_t  n;
    kmp_free_fn free_fn;
    uint64_t  map_len;        /* != 0: bytes is the file mapping itself (no copy was made), released by munmap */
} kmp_frames;
/* alloc_fn == NULL: no copy at all -- bytes is the read-only mapping of the file (a host-to-device copy
 * straight from it runs at PCIe speed on the MI355X hosts, profiles/r01_h2d_probe.txt); with an allocator
 * the file is copied into its memory by several threads. */
int  kmp_frames_from_pcap(const char *path, kmp_alloc_fn alloc_fn, kmp_free_fn free_fn, kmp_frames *out,
                          char errbuf[KMP_PCAP_ERRBUF]);
void kmp_frames_free(kmp_frames *f);

/* ---- streamed capture: batches -----------------------------------------------------------------
 * Replaces the producer of openmp_task.c:126-155 (read up to N packets, extract, hand the batch to
 * a task).  The caller owns the (pinned) buffers; a batch ends when the next payload would not fit
 * in cap_bytes / cap_pkts.  The batch is a packed arena in the sense of kmpgpu.h. */
typedef struct kmp_batch_reader kmp_batch_reader;
kmp_batch_reader *kmp_batch_open(const char *path, int proto, char errbuf[KMP_PCAP_ERRBUF]);
/* Returns the number of payloads stored (0 = end of capture), or a negative KMPHOST_E* code
 * (KMPHOST_EINVAL: a single payload is larger than cap_bytes).  *used_bytes = arena bytes to upload
 * (slack included), *frames += records read. */
int64_t kmp_batch_next(kmp_batch_reader *r, uint8_t *arena, uint64_t cap_bytes, uint64_t *off, uint32_t *len,
                       uint64_t cap_pkts, uint64_t *used_bytes, uint64_t *frames);
/* The same producer with the extraction left to the GPU (kmpgpu_load_frames): the next records of the capture whose bytes
 * span at most max_span_bytes of the file (at least one record, at most cap_frames).  Only the record headers are read;
 * frame_off[f] / frame_caplen[f] locate the frames inside the buffer kmp_batch_file() returns (the mapped capture itself:
 * nothing is copied here).  Returns the number of frames (0 = end of capture).  A reader serves either kind of batch, not both. */
int64_t kmp_batch_next_frames(kmp_batch_reader *r, uint64_t max_span_bytes, uint64_t *frame_off, uint32_t *frame_caplen,
                              uint64_t cap_frames);
const uint8_t *kmp_batch_file(const kmp_batch_reader *r, uint64_t *nbytes);
/* memcpy by several threads (the CPUs this process may use, at most 16; KMPHOST_THREADS): stages a batch of raw frames from the mapped
 * capture into a pinned buffer -- one bulk copy per batch, no per-packet work. */
void kmp_copy_bytes(uint8_t *dst, const uint8_t *src, uint64_t n);
void kmp_batch_close(kmp_batch_reader *r);

/* Synthetic fill on the host (same bytes as the device generator, kmp_synth.h). */
void kmp_synth_fill_host(uint8_t *arena, const uint64_t *off, const uint32_t *len, uint64_t first_pkt_id,
                         uint64_t n, const kmp_synth_params *sp, int threads);
/* Number of packets among ids [first, first+n) that carry the needle. */
uint64_t kmp_synth_count_planted(const uint32_t *len, uint32_t fixed_len, uint64_t first_pkt_id, uint64_t n,
                                 const kmp_synth_params *sp);

/* ---- report ---------------------------------------------------------------------------------
 * serial.c:163-169: header line, "%s: %d times!" for every pattern with a non-zero count in file
 * order, then "Elapsed time = %f seconds". */
void kmp_report(FILE *fp, const kmp_patterns *pats, const uint64_t *counts, double elapsed_seconds);

/* Write a classic little-endian pcap of Ethernet/IPv4/UDP frames around the arena's payloads
 * (test + benchmark tooling: proves arena-route == pcap-route). */
int kmp_write_udp_pcap(const char *path, const uint8_t *arena, const uint64_t *off, const uint32_t *len, uint64_t n);
/* The same in parts, for payloads that arrive arena by arena (the shards of a packet export): append == 0 starts the file (global
 * header, then these n frames), append != 0 adds n frames behind what the file holds; first_record = the number of frames written
 * before, which the record timestamps count on.  Parts written in order give byte for byte the file of one kmp_write_udp_pcap call
 * over all payloads.  n == 0 with append == 0 leaves a valid capture without frames. */
int kmp_write_udp_pcap_part(const char *path, int append, const uint8_t *arena, const uint64_t *off, const uint32_t *len, uint64_t n,
                            uint64_t first_record);

#ifdef __cplusplus
}
#endif
#endif /* KMPHOST_H */
