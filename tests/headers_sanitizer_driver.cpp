/* Built with -fsanitize=address,undefined by tests/test_headers_host.py: drives kmp_pack_headers and the n_hdr entries of the rules,
 * relations and chains packers (csrc/kmp_rowtables.cpp) without a device.  Every expected table below is written out by hand from the
 * description of the device form in csrc/kmp_rowtables.h, none is computed by the code under test. */
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "kmp_rowtables.h"

typedef std::vector<uint32_t> Words;

static int g_failed = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "CHECK failed: %s (line %d)\n", #c, __LINE__); g_failed++; } } while (0)

static const uint32_t N = KMPGPU_RULE_NOT;

static bool refused(int rc, const std::string &msg, const char *text)
{
    const bool ok = rc == KMPGPU_EINVAL && msg == text;
    if (!ok) fprintf(stderr, "rc %d, message '%s' (wanted '%s')\n", rc, msg.c_str(), text);
    return ok;
}

static kmpgpu_header any_header(void)
{
    kmpgpu_header h;
    memset(&h, 0, sizeof h);
    h.sport_hi = h.dport_hi = 0xFFFFu;
    h.len_hi = 0xFFFFFFFFu;
    h.flags = KMPGPU_HDR_ANY_PROTO;
    return h;
}

static void headers(void)
{
    std::vector<kmpgpu_header> h(3, any_header());
    /* udp 10.1.2.3/8 1024: -> 192.168.0.0/16 53, 1:1500 -- the addresses are stored masked */
    h[1].flags = 0; h[1].proto = 17;
    h[1].src_ip = 0x0A010203u; h[1].src_mask = 0xFF000000u; h[1].dst_ip = 0xC0A80000u; h[1].dst_mask = 0xFFFF0000u;
    h[1].sport_lo = 1024; h[1].sport_hi = 65535; h[1].dport_lo = 53; h[1].dport_hi = 53; h[1].len_lo = 1; h[1].len_hi = 1500;
    /* 6 <> with a non-contiguous mask, port 0, length 0:0 */
    h[2].flags = KMPGPU_HDR_BIDIR; h[2].proto = 6;
    h[2].src_ip = 0xFFFFFFFFu; h[2].src_mask = 0x00FF00FFu; h[2].dst_ip = 0x01020304u; h[2].dst_mask = 0xFFFFFFFFu;
    h[2].sport_lo = 0; h[2].sport_hi = 0; h[2].len_lo = 0; h[2].len_hi = 0;
    const Words want = {
        0, 0, 0, 0,                                   0xFFFF0000u, 0xFFFF0000u, 0, 0xFFFFFFFFu,          0x100u, 0, 0, 0,
        0x0A000000u, 0xFF000000u, 0xC0A80000u, 0xFFFF0000u,  0xFFFF0400u, 0x00350035u, 1, 1500,         17u, 0, 0, 0,
        0x00FF00FFu, 0x00FF00FFu, 0x01020304u, 0xFFFFFFFFu,  0x00000000u, 0xFFFF0000u, 0, 0,             0x206u, 0, 0, 0,
    };
    Words got;
    std::string msg;
    CHECK(kmp_pack_headers(h.data(), 3, 8, 1, 1, &got, &msg) == KMPGPU_OK);
    CHECK(got == want);

    /* every refusal; the table comes back empty */
    CHECK(refused(kmp_pack_headers(nullptr, 1, 8, 0, 0, &got, &msg), msg, "kmpgpu_set_headers: h is NULL"));
    CHECK(got.empty());
    std::vector<kmpgpu_header> b = h;
    b[1].sport_lo = 7; b[1].sport_hi = 6;
    CHECK(refused(kmp_pack_headers(b.data(), 3, 8, 0, 0, &got, &msg), msg, "kmpgpu_set_headers: predicate 1: source port 7 lies above 6"));
    b = h; b[2].dport_lo = 65535; b[2].dport_hi = 65534;
    CHECK(refused(kmp_pack_headers(b.data(), 3, 8, 0, 0, &got, &msg), msg, "kmpgpu_set_headers: predicate 2: destination port 65535 lies above 65534"));
    b = h; b[0].len_lo = 0xFFFFFFFFu; b[0].len_hi = 0xFFFFFFFEu;
    CHECK(refused(kmp_pack_headers(b.data(), 3, 8, 0, 0, &got, &msg), msg, "kmpgpu_set_headers: predicate 0: length 4294967295 lies above 4294967294"));
    b = h; b[1].flags = 4;
    CHECK(refused(kmp_pack_headers(b.data(), 3, 8, 0, 0, &got, &msg), msg, "kmpgpu_set_headers: predicate 1: unknown flag bits 0x4"));
    b = h; b[2].flags = 0x83;
    CHECK(refused(kmp_pack_headers(b.data(), 3, 8, 0, 0, &got, &msg), msg, "kmpgpu_set_headers: predicate 2: unknown flag bits 0x80"));
    b = h; b[0].reserved = 9;
    CHECK(refused(kmp_pack_headers(b.data(), 3, 8, 0, 0, &got, &msg), msg, "kmpgpu_set_headers: predicate 0: reserved is 9, not 0"));
    CHECK(got.empty());

    /* the 2^31 bound is checked on the counts alone, before an array is read: one valid predicate stands for 2^31 - 11 of them */
    CHECK(refused(kmp_pack_headers(h.data(), 0x7FFFFFF5u, 8, 2, 1, &got, &msg), msg,
                  "kmpgpu_set_headers: 8 patterns + 2 relations + 1 chains + 2147483637 header predicates do not fit the 2^31 rows a rule term can name"));
    CHECK(refused(kmp_pack_headers(h.data(), 1, 0x7FFFFFFFu, 0, 0, &got, &msg), msg,
                  "kmpgpu_set_headers: 2147483647 patterns + 0 relations + 0 chains + 1 header predicates do not fit the 2^31 rows a rule term can name"));
    /* one below it passes the bound (3 predicates, 2^31 - 4 patterns: 2^31 - 1 rows) */
    CHECK(kmp_pack_headers(h.data(), 3, 0x7FFFFFFCu, 0, 0, &got, &msg) == KMPGPU_OK && got == want);
}

/* the n_hdr entries of the other packers: the rules' terms reach the predicates' rows, the relations' and chains' bound counts them in,
 * and the entries without n_hdr are the ones with 0 */
static void siblings(void)
{
    /* 8 patterns + 1 relation + 1 chain + 2 predicates = rows 0 .. 11 */
    const Words off = {0, 2, 3}, terms = {10, N | 11, N | 10};
    const Words want_heads = {0, 0, 10, N | 11,  0, 0, N | 10, N | 10};
    Words heads, quads;
    std::string msg;
    CHECK(kmp_pack_rules(off.data(), terms.data(), 2, 8, 1, 1, 2, &heads, &quads, &msg) == KMPGPU_OK);
    CHECK(heads == want_heads && quads.empty());
    CHECK(refused(kmp_pack_rules(off.data(), terms.data(), 2, 8, 1, 1, 1, &heads, &quads, &msg), msg,
                  "kmpgpu_set_rules: rule 0: term 1 names row 11 of 8 patterns + 1 relations + 1 chains + 1 header predicates"));
    /* without n_hdr a predicate's row is no row, and the message is the one it always was */
    CHECK(refused(kmp_pack_rules(off.data(), terms.data(), 2, 8, 1, 1, &heads, &quads, &msg), msg,
                  "kmpgpu_set_rules: rule 0: term 0 names row 10 of 8 patterns + 1 relations + 1 chains"));
    CHECK(refused(kmp_pack_rules(off.data(), terms.data(), 2, 8, 1, 1, 0, &heads, &quads, &msg), msg,
                  "kmpgpu_set_rules: rule 0: term 0 names row 10 of 8 patterns + 1 relations + 1 chains"));

    const uint8_t fold[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const kmpgpu_relation rel = {1, 2, -3, 4};
    Words r;
    CHECK(kmp_pack_relations(&rel, 1, 8, 1, 5, fold, &r, &msg) == KMPGPU_OK && r == Words({1, 2, 0xFFFFFFFDu, 4}));
    CHECK(refused(kmp_pack_relations(&rel, 1, 8, 0, 0x7FFFFFF7u, fold, &r, &msg), msg,
                  "kmpgpu_set_relations: 8 patterns + 1 relations + the header predicates do not fit the 2^31 rows a rule term can name"));
    CHECK(kmp_pack_relations(&rel, 1, 8, 0, 0x7FFFFFF6u, fold, &r, &msg) == KMPGPU_OK);
    CHECK(kmp_pack_relations(&rel, 1, 8, 1, fold, &r, &msg) == KMPGPU_OK && r == Words({1, 2, 0xFFFFFFFDu, 4}));

    const Words coff = {0, 2};
    const kmpgpu_chain_link links[2] = {{1, INT32_MIN, INT32_MAX}, {2, 0, 5}};
    Words c;
    CHECK(kmp_pack_chains(coff.data(), links, 1, 8, 1, 3, fold, &c, &msg) == KMPGPU_OK && c.size() == 4u * KMPGPU_CHAIN_MAX);
    CHECK(refused(kmp_pack_chains(coff.data(), links, 1, 8, 1, 0x7FFFFFF6u, fold, &c, &msg), msg,
                  "kmpgpu_set_chains: 8 patterns + 1 relations + 1 chains + the header predicates do not fit the 2^31 rows a rule term can name"));
    CHECK(kmp_pack_chains(coff.data(), links, 1, 8, 1, 0x7FFFFFF5u, fold, &c, &msg) == KMPGPU_OK);
}

int main(void)
{
    headers();
    siblings();
    if (g_failed) { fprintf(stderr, "%d checks failed\n", g_failed); return 1; }
    printf("headers driver ok\n");
    return 0;
}
