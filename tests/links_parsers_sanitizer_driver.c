/* The links-file parser and the rules-file parser with l<q> terms (csrc/host/kmphost.c) and the buffer words of a links file
 * (csrc/host/kmp_cli_links.h) on their own, for AddressSanitizer + UBSan (tests/test_links_host.py).  Files are written to the directory
 * given as argv[1]; buffer words are handed over in heap blocks of exactly their size, so a read behind a terminator is seen. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "kmphost.h"
#include "kmp_cli_links.h"

static int g_failed = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "CHECK failed: %s (line %d)\n", #c, __LINE__); g_failed++; } } while (0)

static char g_path[1024];

static const char *file_with(const char *dir, const char *text)
{
    snprintf(g_path, sizeof g_path, "%s/links_driver.txt", dir);
    FILE *fp = fopen(g_path, "wb");
    if (!fp) { perror(g_path); exit(2); }
    fwrite(text, 1, strlen(text), fp);
    fclose(fp);
    return g_path;
}

/* 5 patterns, 1 relation, 1 chain, 1 header predicate, 1 byte test, 2 expressions: rows 0 .. 10 */
static int links_of(const char *dir, const char *text, kmp_links *l, char *err)
{
    return kmp_links_parse(file_with(dir, text), 5, 1, 1, 1, 1, 2, l, err);
}

static void links_files(const char *dir)
{
    kmp_links l;
    char err[KMP_LINKS_ERRBUF];
    CHECK(links_of(dir, "# comment\n\nhttp:body 4\n  dns:qname,tcp   r0\ndecode:percent c0\nbase64:16,url b0\nhttp:uri x1\nhttp:uri h0", &l, err) == KMPHOST_OK);
    CHECK(l.n == 6);
    if (l.n == 6) {
        CHECK(!strcmp(l.buffer[0], "http:body") && l.term[0] == 4);
        CHECK(!strcmp(l.buffer[1], "dns:qname,tcp") && l.term[1] == 5);
        CHECK(!strcmp(l.buffer[2], "decode:percent") && l.term[2] == 6);
        CHECK(!strcmp(l.buffer[3], "base64:16,url") && l.term[3] == 8);
        CHECK(!strcmp(l.buffer[4], "http:uri") && l.term[4] == 10);
        CHECK(!strcmp(l.buffer[5], "http:uri") && l.term[5] == 7);
    }
    kmp_links_free(&l);
    kmp_links_free(&l);                                                        /* twice: harmless */
    CHECK(links_of(dir, "", &l, err) == KMPHOST_OK && l.n == 0);
    kmp_links_free(&l);
    /* more links than the first allocation holds */
    char *many = (char *)malloc(100 * 16 + 1);
    many[0] = 0;
    for (int i = 0; i < 100; i++) sprintf(many + strlen(many), "http:body %d\n", i % 5);
    CHECK(links_of(dir, many, &l, err) == KMPHOST_OK && l.n == 100 && l.term[99] == 4);
    free(many);
    kmp_links_free(&l);
    static const char *const bad[][2] = {
        {"http:body !3\n", "line 1: a link's term is not negated: the rule that names the link negates it"},
        {"http:body 1\nhttp:body l0\n", "line 2: a link's term names no link"},
        {"http:body 5\n", "line 1: pattern index 5, but there are 5 patterns"},
        {"http:body x2\n", "line 1: expression index 2, but there are 2 expressions"},
        {"http:body\n", "line 1: 'http:body' without a term: a line is <buffer> <term>"},
        {"http:body", "line 1: 'http:body' without a term: a line is <buffer> <term>"},
        {"http:body 1 r0\n", "line 1: 2 terms: a link is one term"},
        {"http:body 1x\n", "line 1: '1x' is not a pattern index or r<relation index> or c<chain index> or h<header index> or b<byte test index> or x<expression index>"},
        {"0123456789012345678901234567890123456789012345678901234567890123 1\n", "line 1: a buffer word of 64 characters: at most 63"}};
    for (size_t i = 0; i < sizeof bad / sizeof bad[0]; i++) {
        CHECK(links_of(dir, bad[i][0], &l, err) == KMPHOST_EINVAL);
        if (strcmp(err, bad[i][1])) { fprintf(stderr, "'%s' (wanted '%s')\n", err, bad[i][1]); g_failed++; }
        CHECK(l.n == 0 && !l.buffer && !l.term);
    }
    /* 63 characters fit */
    CHECK(links_of(dir, "012345678901234567890123456789012345678901234567890123456789012 1\n", &l, err) == KMPHOST_OK && l.n == 1 && strlen(l.buffer[0]) == 63);
    kmp_links_free(&l);
    CHECK(kmp_links_parse("/no/such/dir/links.txt", 5, 0, 0, 0, 0, 0, &l, err) == KMPHOST_EIO);
}

static void rules_files(const char *dir)
{
    kmp_rules r;
    char err[KMP_RULES_ERRBUF];
    /* rows: 5 patterns + 1 + 1 + 1 + 1 + 2 = 11, then 3 links = rows 11 .. 13 */
    CHECK(kmp_rules_parse_links(file_with(dir, "l0 !l2 3\nx1 l1\n"), 5, 1, 1, 1, 1, 2, 3, &r, err) == KMPHOST_OK);
    CHECK(r.n == 2);
    if (r.n == 2) {
        CHECK(r.off[0] == 0 && r.off[1] == 3 && r.off[2] == 5);
        CHECK(r.terms[0] == 11 && r.terms[1] == (13u | KMP_RULE_NOT) && r.terms[2] == 3 && r.terms[3] == 10 && r.terms[4] == 12);
    }
    kmp_rules_free(&r);
    CHECK(kmp_rules_parse_links(file_with(dir, "l3\n"), 5, 1, 1, 1, 1, 2, 3, &r, err) == KMPHOST_EINVAL);
    CHECK(!strcmp(err, "line 1: link index 3, but there are 3 links"));
    CHECK(kmp_rules_parse_links(file_with(dir, "0 l\n"), 5, 0, 0, 0, 0, 0, 3, &r, err) == KMPHOST_EINVAL);
    CHECK(!strcmp(err, "line 1: 'l' is not a pattern index or l<link index>"));
    CHECK(kmp_rules_parse_links(file_with(dir, "!l99999999999999999999\n"), 5, 0, 0, 0, 0, 0, 3, &r, err) == KMPHOST_EINVAL);
    /* without links the letter is no term, and the entry without them says the same */
    CHECK(kmp_rules_parse_links(file_with(dir, "l0\n"), 5, 1, 1, 1, 1, 2, 0, &r, err) == KMPHOST_EINVAL);
    char err2[KMP_RULES_ERRBUF];
    CHECK(kmp_rules_parse_rx(g_path, 5, 1, 1, 1, 1, 2, &r, err2) == KMPHOST_EINVAL && !strcmp(err, err2));
    /* the row bound counts the links */
    CHECK(kmp_rules_parse_links(file_with(dir, "0\n"), 5, 0, 0, 0, 0, 0, 0x7FFFFFFBu, &r, err) == KMPHOST_EINVAL);
    CHECK(strstr(err, "2147483643 links do not fit the 2^31 rows") != NULL);
    CHECK(kmp_rules_parse_links(g_path, 5, 0, 0, 0, 0, 0, 0x7FFFFFFAu, &r, err) == KMPHOST_OK);
    kmp_rules_free(&r);
}

static int buffer_word(const char *s, kmp_cli_link_buffer *b)
{
    char *copy = (char *)malloc(strlen(s) + 1);
    memcpy(copy, s, strlen(s) + 1);
    const int ok = kmp_cli_parse_link_buffer(copy, b);
    free(copy);
    return ok;
}

static void buffer_words(void)
{
    kmp_cli_link_buffer a, b;
    CHECK(buffer_word("http:body", &a) && a.kind == KMP_CLI_LINK_HTTP && a.field == KMP_CLI_FIELD_BODY);
    CHECK(buffer_word("http:uri", &b) && b.field == KMP_CLI_FIELD_URI && !kmp_cli_link_buffer_same(&a, &b));
    CHECK(buffer_word("http:body", &b) && kmp_cli_link_buffer_same(&a, &b));
    CHECK(buffer_word("dns:qname", &a) && a.kind == KMP_CLI_LINK_DNS && a.field == KMP_CLI_DNS_QNAME && !a.flag);
    CHECK(buffer_word("dns:qname,tcp", &b) && b.flag == 1 && !kmp_cli_link_buffer_same(&a, &b));
    CHECK(buffer_word("decode:percent", &a) && a.kind == KMP_CLI_LINK_DECODE && a.field == KMP_CLI_DECODE_PERCENT);
    CHECK(buffer_word("decode:percent+plus", &b) && b.field == KMP_CLI_DECODE_PLUS);
    CHECK(buffer_word("base64:16", &a) && a.kind == KMP_CLI_LINK_BASE64 && a.min_run == 16 && !a.flag);
    CHECK(buffer_word("base64:016,url", &b) && b.min_run == 16 && b.flag == 1 && !kmp_cli_link_buffer_same(&a, &b));
    CHECK(buffer_word("base64:016", &b) && kmp_cli_link_buffer_same(&a, &b));                  /* the same buffer, spelt otherwise */
    static const char *const bad[] = {"", "http", "http:", "http:cookie", "HTTP:body", "body", "dns:", "dns:qname,udp", "decode:", "decode:plus",
                                      "base64:", "base64:3", "base64:256", "base64:16,", "base64:99999999999999999999", "tls:sni", "http:body "};
    for (size_t i = 0; i < sizeof bad / sizeof bad[0]; i++) CHECK(!buffer_word(bad[i], &a));
    CHECK(!kmp_cli_parse_link_buffer(NULL, &a));
}

int main(int argc, char *argv[])
{
    if (argc != 2) { fprintf(stderr, "usage: driver <scratch directory>\n"); return 2; }
    links_files(argv[1]);
    rules_files(argv[1]);
    buffer_words();
    if (g_failed) { fprintf(stderr, "%d checks failed\n", g_failed); return 1; }
    printf("links parsers driver ok\n");
    return 0;
}
