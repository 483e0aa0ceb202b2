/* Stand-alone driver of the relation parsers of the host library (kmp_relations_parse, kmp_rules_parse_rel, kmp_rules_parse) for a
 * build under -fsanitize=address,undefined (tests/test_relations_host.py):
 *     driver <n_patterns> <relations file> [<rules file>]
 * prints "relations rc=<rc> n=<n> msg=<errbuf>", one "rel <a> <b> <dmin> <dmax>" line per relation, then for a rules file
 * "rules rc=<rc> n=<n> msg=<errbuf>" with one "rule <term> ..." line per rule (parsed with the relations' count) and
 * "plain rc=<rc> msg=<errbuf>" (the same file without relations).  Exit code 0 whatever the parsers return. */
#include <stdio.h>
#include <stdlib.h>

#include "kmphost.h"

int main(int argc, char *argv[])
{
    if (argc < 3) { fprintf(stderr, "usage: driver <n_patterns> <relations file> [<rules file>]\n"); return 2; }
    const uint32_t n_patterns = (uint32_t)strtoul(argv[1], NULL, 10);
    char err[KMP_RELATIONS_ERRBUF];
    kmp_relations rel;
    int rc = kmp_relations_parse(argv[2], n_patterns, &rel, err);
    printf("relations rc=%d n=%u msg=%s\n", rc, rel.n, err);
    for (uint32_t q = 0; q < rel.n; q++) printf("rel %u %u %d %d\n", rel.rel[q].a, rel.rel[q].b, rel.rel[q].dmin, rel.rel[q].dmax);
    if (argc > 3) {
        char rerr[KMP_RULES_ERRBUF];
        kmp_rules rules;
        rc = kmp_rules_parse_rel(argv[3], n_patterns, rel.n, &rules, rerr);
        printf("rules rc=%d n=%u msg=%s\n", rc, rules.n, rerr);
        for (uint32_t r = 0; r < rules.n; r++) {
            printf("rule");
            for (uint32_t j = rules.off[r]; j < rules.off[r + 1]; j++) printf(" %u", rules.terms[j]);
            printf("\n");
        }
        kmp_rules_free(&rules);
        rc = kmp_rules_parse(argv[3], n_patterns, &rules, rerr);
        printf("plain rc=%d msg=%s\n", rc, rerr);
        kmp_rules_free(&rules);
    }
    kmp_relations_free(&rel);
    kmp_relations_free(&rel);                          /* freeing twice is harmless */
    printf("relations driver ok\n");
    return 0;
}
