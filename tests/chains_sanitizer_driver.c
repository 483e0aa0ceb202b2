/* Stand-alone driver of the chain parsers of the host library (kmp_chains_parse, kmp_rules_parse_terms, kmp_rules_parse_rel) for a
 * build under -fsanitize=address,undefined (tests/test_chains_host.py):
 *     driver <n_patterns> <n_relations> <chains file> [<rules file>]
 * prints "chains rc=<rc> n=<n> msg=<errbuf>", one "chain <dmin> <dmax> <p> ..." line per chain (three numbers per link, the first
 * link's open bounds included), then for a rules file "rules rc=<rc> n=<n> msg=<errbuf>" with one "rule <term> ..." line per rule (parsed with the
 * chains' count) and "rel rc=<rc> msg=<errbuf>" (the same file without chains).  Exit code 0 whatever the parsers return. */
#include <stdio.h>
#include <stdlib.h>

#include "kmphost.h"

int main(int argc, char *argv[])
{
    if (argc < 4) { fprintf(stderr, "usage: driver <n_patterns> <n_relations> <chains file> [<rules file>]\n"); return 2; }
    const uint32_t n_patterns = (uint32_t)strtoul(argv[1], NULL, 10), n_relations = (uint32_t)strtoul(argv[2], NULL, 10);
    char err[KMP_CHAINS_ERRBUF];
    kmp_chains ch;
    int rc = kmp_chains_parse(argv[3], n_patterns, &ch, err);
    printf("chains rc=%d n=%u msg=%s\n", rc, ch.n, err);
    for (uint32_t c = 0; c < ch.n; c++) {
        printf("chain");
        for (uint32_t j = ch.off[c]; j < ch.off[c + 1]; j++) printf(" %d %d %u", ch.links[j].dmin, ch.links[j].dmax, ch.links[j].pattern);
        printf("\n");
    }
    if (argc > 4) {
        char rerr[KMP_RULES_ERRBUF];
        kmp_rules rules;
        rc = kmp_rules_parse_terms(argv[4], n_patterns, n_relations, ch.n, &rules, rerr);
        printf("rules rc=%d n=%u msg=%s\n", rc, rules.n, rerr);
        for (uint32_t r = 0; r < rules.n; r++) {
            printf("rule");
            for (uint32_t j = rules.off[r]; j < rules.off[r + 1]; j++) printf(" %u", rules.terms[j]);
            printf("\n");
        }
        kmp_rules_free(&rules);
        rc = kmp_rules_parse_rel(argv[4], n_patterns, n_relations, &rules, rerr);
        printf("rel rc=%d msg=%s\n", rc, rerr);
        kmp_rules_free(&rules);
    }
    kmp_chains_free(&ch);
    kmp_chains_free(&ch);                              /* freeing twice is harmless */
    printf("chains driver ok\n");
    return 0;
}
