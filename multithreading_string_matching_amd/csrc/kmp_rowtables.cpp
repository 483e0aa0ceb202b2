/*
 * kmp_rowtables.cpp -- the tables of the rules, windows, relations, chains, header predicates and byte tests as the kernels read them (kmp_rowtables.h; the expressions' packer, kmp_pack_regexes, sits with their compiler in kmp_regex.cpp).  Host code only.
 */
#include "kmp_rowtables.h"

#include <stdarg.h>
#include <stdio.h>

namespace {

int refuse(std::string *msg, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    *msg = buf;
    return KMPGPU_EINVAL;
}

/* bit 31: the pattern's bytes are compared in the folded copy of the arena */
uint32_t fold_bit(const uint8_t *pat_fold, uint32_t pattern) { return pattern | ((uint32_t)(pat_fold[pattern] != 0) << 31); }

}  // namespace

int kmp_pack_rules(const uint32_t *rule_off, const uint32_t *terms, uint32_t n_rules, uint32_t n_pat, uint32_t n_rel, uint32_t n_chains,
                   std::vector<uint32_t> *heads, std::vector<uint32_t> *quads, std::string *msg)
{
    return kmp_pack_rules(rule_off, terms, n_rules, n_pat, n_rel, n_chains, 0u, heads, quads, msg);
}

int kmp_pack_rules(const uint32_t *rule_off, const uint32_t *terms, uint32_t n_rules, uint32_t n_pat, uint32_t n_rel, uint32_t n_chains,
                   uint32_t n_hdr, std::vector<uint32_t> *heads, std::vector<uint32_t> *quads, std::string *msg)
{
    return kmp_pack_rules(rule_off, terms, n_rules, n_pat, n_rel, n_chains, n_hdr, 0u, heads, quads, msg);
}

int kmp_pack_rules(const uint32_t *rule_off, const uint32_t *terms, uint32_t n_rules, uint32_t n_pat, uint32_t n_rel, uint32_t n_chains,
                   uint32_t n_hdr, uint32_t n_bt, std::vector<uint32_t> *heads, std::vector<uint32_t> *quads, std::string *msg)
{
    return kmp_pack_rules(rule_off, terms, n_rules, n_pat, n_rel, n_chains, n_hdr, n_bt, 0u, heads, quads, msg);
}

int kmp_pack_rules(const uint32_t *rule_off, const uint32_t *terms, uint32_t n_rules, uint32_t n_pat, uint32_t n_rel, uint32_t n_chains,
                   uint32_t n_hdr, uint32_t n_bt, uint32_t n_rx, std::vector<uint32_t> *heads, std::vector<uint32_t> *quads, std::string *msg)
{
    return kmp_pack_rules(rule_off, terms, n_rules, n_pat, n_rel, n_chains, n_hdr, n_bt, n_rx, 0u, heads, quads, msg);
}

int kmp_pack_rules(const uint32_t *rule_off, const uint32_t *terms, uint32_t n_rules, uint32_t n_pat, uint32_t n_rel, uint32_t n_chains,
                   uint32_t n_hdr, uint32_t n_bt, uint32_t n_rx, uint32_t n_links, std::vector<uint32_t> *heads, std::vector<uint32_t> *quads,
                   std::string *msg)
{
    heads->clear(); quads->clear();
    if (!rule_off || !terms) return refuse(msg, "kmpgpu_set_rules: NULL rule arrays");
    if (rule_off[0] != 0) return refuse(msg, "kmpgpu_set_rules: rule_off[0] is %u, not 0", rule_off[0]);
    const uint64_t n_rows = (uint64_t)n_pat + n_rel + n_chains + n_hdr + n_bt + n_rx + n_links;  /* (< 2^31: the other packers without the links, kmpgpu_set_links and links_fit in every setter with them) */
    std::vector<uint32_t> ord;
    for (uint32_t r = 0; r < n_rules; r++) {
        if (rule_off[r + 1] < rule_off[r]) return refuse(msg, "kmpgpu_set_rules: rule_off decreases at rule %u", r);
        if (rule_off[r + 1] == rule_off[r]) return refuse(msg, "kmpgpu_set_rules: rule %u has no terms", r);
        ord.clear();
        for (int neg = 0; neg < 2; neg++)
            for (uint32_t j = rule_off[r]; j < rule_off[r + 1]; j++) {
                if ((terms[j] & ~KMPGPU_RULE_NOT) >= n_rows && n_links)
                    return refuse(msg, "kmpgpu_set_rules: rule %u: term %u names row %u of %u patterns + %u relations + %u chains + %u header predicates + %u byte tests + %u expressions + %u links",
                                  r, j - rule_off[r], terms[j] & ~KMPGPU_RULE_NOT, n_pat, n_rel, n_chains, n_hdr, n_bt, n_rx, n_links);
                if ((terms[j] & ~KMPGPU_RULE_NOT) >= n_rows && n_rx)
                    return refuse(msg, "kmpgpu_set_rules: rule %u: term %u names row %u of %u patterns + %u relations + %u chains + %u header predicates + %u byte tests + %u expressions",
                                  r, j - rule_off[r], terms[j] & ~KMPGPU_RULE_NOT, n_pat, n_rel, n_chains, n_hdr, n_bt, n_rx);
                if ((terms[j] & ~KMPGPU_RULE_NOT) >= n_rows && n_bt)
                    return refuse(msg, "kmpgpu_set_rules: rule %u: term %u names row %u of %u patterns + %u relations + %u chains + %u header predicates + %u byte tests",
                                  r, j - rule_off[r], terms[j] & ~KMPGPU_RULE_NOT, n_pat, n_rel, n_chains, n_hdr, n_bt);
                if ((terms[j] & ~KMPGPU_RULE_NOT) >= n_rows && n_hdr)
                    return refuse(msg, "kmpgpu_set_rules: rule %u: term %u names row %u of %u patterns + %u relations + %u chains + %u header predicates",
                                  r, j - rule_off[r], terms[j] & ~KMPGPU_RULE_NOT, n_pat, n_rel, n_chains, n_hdr);
                if ((terms[j] & ~KMPGPU_RULE_NOT) >= n_rows)
                    return refuse(msg, "kmpgpu_set_rules: rule %u: term %u names row %u of %u patterns + %u relations + %u chains", r,
                                  j - rule_off[r], terms[j] & ~KMPGPU_RULE_NOT, n_pat, n_rel, n_chains);
                if (((terms[j] & KMPGPU_RULE_NOT) != 0) == (neg != 0)) ord.push_back(terms[j]);
            }
        /* filled up with a term that is loaded at the same time: a repeated term changes nothing */
        if (ord.size() < 2) ord.push_back(ord[0]);
        while ((ord.size() - 2) % 4) ord.push_back(ord[ord.size() - (ord.size() - 2) % 4]);
        const uint64_t q0 = quads->size() / 4, q1 = q0 + (ord.size() - 2) / 4;
        if (q1 > 0xFFFFFFFFull) return refuse(msg, "kmpgpu_set_rules: too many terms");
        heads->insert(heads->end(), {(uint32_t)q0, (uint32_t)q1, ord[0], ord[1]});
        quads->insert(quads->end(), ord.begin() + 2, ord.end());
    }
    return KMPGPU_OK;
}

int kmp_pack_windows(const uint32_t *first, const uint32_t *last, uint32_t n_windows, uint32_t n_pat, std::vector<uint32_t> *windows,
                     std::string *msg)
{
    windows->clear();
    if (n_windows != n_pat) return refuse(msg, "kmpgpu_set_windows: %u windows for %u patterns", n_windows, n_pat);
    if (!first || !last) return refuse(msg, "kmpgpu_set_windows: NULL window arrays");
    bool all_default = true;
    for (uint32_t i = 0; i < n_pat; i++) {
        if (first[i] > last[i]) return refuse(msg, "kmpgpu_set_windows: pattern %u: first %u lies behind last %u", i, first[i], last[i]);
        windows->insert(windows->end(), {first[i], last[i]});
        all_default = all_default && first[i] == 0u && last[i] == 0xFFFFFFFFu;
    }
    if (all_default) windows->clear();
    return KMPGPU_OK;
}

int kmp_pack_relations(const kmpgpu_relation *rel, uint32_t n_rel, uint32_t n_pat, uint32_t n_chains, const uint8_t *pat_fold,
                       std::vector<uint32_t> *relations, std::string *msg)
{
    return kmp_pack_relations(rel, n_rel, n_pat, n_chains, 0u, pat_fold, relations, msg);
}

int kmp_pack_relations(const kmpgpu_relation *rel, uint32_t n_rel, uint32_t n_pat, uint32_t n_chains, uint32_t n_hdr, const uint8_t *pat_fold,
                       std::vector<uint32_t> *relations, std::string *msg)
{
    return kmp_pack_relations(rel, n_rel, n_pat, n_chains, n_hdr, 0u, pat_fold, relations, msg);
}

int kmp_pack_relations(const kmpgpu_relation *rel, uint32_t n_rel, uint32_t n_pat, uint32_t n_chains, uint32_t n_hdr, uint32_t n_bt,
                       const uint8_t *pat_fold, std::vector<uint32_t> *relations, std::string *msg)
{
    return kmp_pack_relations(rel, n_rel, n_pat, n_chains, n_hdr, n_bt, 0u, pat_fold, relations, msg);
}

int kmp_pack_relations(const kmpgpu_relation *rel, uint32_t n_rel, uint32_t n_pat, uint32_t n_chains, uint32_t n_hdr, uint32_t n_bt,
                       uint32_t n_rx, const uint8_t *pat_fold, std::vector<uint32_t> *relations, std::string *msg)
{
    relations->clear();
    if (!rel) return refuse(msg, "kmpgpu_set_relations: rel is NULL");
    if ((uint64_t)n_pat + n_rel + n_chains + n_hdr + n_bt + n_rx >= (1ull << 31))
        return refuse(msg, "kmpgpu_set_relations: %u patterns + %u relations%s%s%s%s do not fit the 2^31 rows a rule term can name", n_pat, n_rel,
                      n_chains ? " + the chains" : "", n_hdr ? " + the header predicates" : "", n_bt ? " + the byte tests" : "",
                      n_rx ? " + the expressions" : "");
    for (uint32_t q = 0; q < n_rel; q++) {
        const kmpgpu_relation &r = rel[q];
        if (r.a >= n_pat || r.b >= n_pat)
            return refuse(msg, "kmpgpu_set_relations: relation %u names pattern %u of %u", q, r.a >= n_pat ? r.a : r.b, n_pat);
        if (r.dmin > r.dmax) return refuse(msg, "kmpgpu_set_relations: relation %u: dmin %d lies above dmax %d", q, r.dmin, r.dmax);
        relations->insert(relations->end(), {fold_bit(pat_fold, r.a), fold_bit(pat_fold, r.b), (uint32_t)r.dmin, (uint32_t)r.dmax});
    }
    return KMPGPU_OK;
}

int kmp_pack_chains(const uint32_t *chain_off, const kmpgpu_chain_link *links, uint32_t n_chains, uint32_t n_pat, uint32_t n_rel,
                    const uint8_t *pat_fold, std::vector<uint32_t> *chains, std::string *msg)
{
    return kmp_pack_chains(chain_off, links, n_chains, n_pat, n_rel, 0u, pat_fold, chains, msg);
}

int kmp_pack_chains(const uint32_t *chain_off, const kmpgpu_chain_link *links, uint32_t n_chains, uint32_t n_pat, uint32_t n_rel,
                    uint32_t n_hdr, const uint8_t *pat_fold, std::vector<uint32_t> *chains, std::string *msg)
{
    return kmp_pack_chains(chain_off, links, n_chains, n_pat, n_rel, n_hdr, 0u, pat_fold, chains, msg);
}

int kmp_pack_chains(const uint32_t *chain_off, const kmpgpu_chain_link *links, uint32_t n_chains, uint32_t n_pat, uint32_t n_rel,
                    uint32_t n_hdr, uint32_t n_bt, const uint8_t *pat_fold, std::vector<uint32_t> *chains, std::string *msg)
{
    return kmp_pack_chains(chain_off, links, n_chains, n_pat, n_rel, n_hdr, n_bt, 0u, pat_fold, chains, msg);
}

int kmp_pack_chains(const uint32_t *chain_off, const kmpgpu_chain_link *links, uint32_t n_chains, uint32_t n_pat, uint32_t n_rel,
                    uint32_t n_hdr, uint32_t n_bt, uint32_t n_rx, const uint8_t *pat_fold, std::vector<uint32_t> *chains, std::string *msg)
{
    chains->clear();
    if (!chain_off || !links) return refuse(msg, "kmpgpu_set_chains: NULL chain arrays");
    if ((uint64_t)n_pat + n_rel + n_chains + n_hdr + n_bt + n_rx >= (1ull << 31))
        return refuse(msg, "kmpgpu_set_chains: %u patterns + %u relations + %u chains%s%s%s do not fit the 2^31 rows a rule term can name", n_pat, n_rel,
                      n_chains, n_hdr ? " + the header predicates" : "", n_bt ? " + the byte tests" : "", n_rx ? " + the expressions" : "");
    if (chain_off[0] != 0) return refuse(msg, "kmpgpu_set_chains: chain_off[0] is %u, not 0", chain_off[0]);
    for (uint32_t q = 0; q < n_chains; q++) {
        if (chain_off[q + 1] < chain_off[q]) return refuse(msg, "kmpgpu_set_chains: chain_off decreases at chain %u", q);
        const uint32_t n = chain_off[q + 1] - chain_off[q];
        if (n < 2 || n > KMPGPU_CHAIN_MAX) return refuse(msg, "kmpgpu_set_chains: chain %u has %u contents, not 2 .. %d", q, n, KMPGPU_CHAIN_MAX);
        const kmpgpu_chain_link *l = links + chain_off[q];
        if (l[0].dmin != INT32_MIN || l[0].dmax != INT32_MAX)
            return refuse(msg, "kmpgpu_set_chains: chain %u: its first content is relative to nothing and carries no bounds (a window places it)", q);
        for (uint32_t i = 0; i < KMPGPU_CHAIN_MAX; i++) {
            const kmpgpu_chain_link &k = l[i < n ? i : n - 1];
            if (k.pattern >= n_pat) return refuse(msg, "kmpgpu_set_chains: chain %u names pattern %u of %u", q, k.pattern, n_pat);
            if (k.dmin > k.dmax) return refuse(msg, "kmpgpu_set_chains: chain %u: dmin %d lies above dmax %d", q, k.dmin, k.dmax);
            chains->insert(chains->end(), {fold_bit(pat_fold, k.pattern), (uint32_t)k.dmin, (uint32_t)k.dmax, n});
        }
    }
    return KMPGPU_OK;
}

int kmp_pack_headers(const kmpgpu_header *h, uint32_t n_hdr, uint32_t n_pat, uint32_t n_rel, uint32_t n_chains, std::vector<uint32_t> *headers,
                     std::string *msg)
{
    return kmp_pack_headers(h, n_hdr, n_pat, n_rel, n_chains, 0u, headers, msg);
}

int kmp_pack_headers(const kmpgpu_header *h, uint32_t n_hdr, uint32_t n_pat, uint32_t n_rel, uint32_t n_chains, uint32_t n_bt,
                     std::vector<uint32_t> *headers, std::string *msg)
{
    return kmp_pack_headers(h, n_hdr, n_pat, n_rel, n_chains, n_bt, 0u, headers, msg);
}

int kmp_pack_headers(const kmpgpu_header *h, uint32_t n_hdr, uint32_t n_pat, uint32_t n_rel, uint32_t n_chains, uint32_t n_bt, uint32_t n_rx,
                     std::vector<uint32_t> *headers, std::string *msg)
{
    headers->clear();
    if (!h) return refuse(msg, "kmpgpu_set_headers: h is NULL");
    if ((uint64_t)n_pat + n_rel + n_chains + n_hdr + n_bt + n_rx >= (1ull << 31))
        return refuse(msg, "kmpgpu_set_headers: %u patterns + %u relations + %u chains + %u header predicates%s%s do not fit the 2^31 rows a rule term can name",
                      n_pat, n_rel, n_chains, n_hdr, n_bt ? " + the byte tests" : "", n_rx ? " + the expressions" : "");
    for (uint32_t q = 0; q < n_hdr; q++) {
        const kmpgpu_header &p = h[q];
        if (p.sport_lo > p.sport_hi) return refuse(msg, "kmpgpu_set_headers: predicate %u: source port %u lies above %u", q, p.sport_lo, p.sport_hi);
        if (p.dport_lo > p.dport_hi) return refuse(msg, "kmpgpu_set_headers: predicate %u: destination port %u lies above %u", q, p.dport_lo, p.dport_hi);
        if (p.len_lo > p.len_hi) return refuse(msg, "kmpgpu_set_headers: predicate %u: length %u lies above %u", q, p.len_lo, p.len_hi);
        if (p.flags & ~(KMPGPU_HDR_ANY_PROTO | KMPGPU_HDR_BIDIR))
            return refuse(msg, "kmpgpu_set_headers: predicate %u: unknown flag bits 0x%x", q, p.flags & ~(KMPGPU_HDR_ANY_PROTO | KMPGPU_HDR_BIDIR));
        if (p.reserved != 0) return refuse(msg, "kmpgpu_set_headers: predicate %u: reserved is %u, not 0", q, p.reserved);
        headers->insert(headers->end(), {p.src_ip & p.src_mask, p.src_mask, p.dst_ip & p.dst_mask, p.dst_mask,
                                         (uint32_t)p.sport_lo | (uint32_t)p.sport_hi << 16, (uint32_t)p.dport_lo | (uint32_t)p.dport_hi << 16, p.len_lo, p.len_hi,
                                         (uint32_t)p.proto | (uint32_t)p.flags << 8, 0u, 0u, 0u});
    }
    return KMPGPU_OK;
}

int kmp_pack_bytetests(const kmpgpu_bytetest *bt, uint32_t n_bt, uint32_t n_pat, uint32_t n_rel, uint32_t n_chains, uint32_t n_hdr,
                       const uint8_t *pat_fold, std::vector<uint32_t> *tests, uint32_t *n_relative, uint32_t *reach, std::string *msg)
{
    return kmp_pack_bytetests(bt, n_bt, n_pat, n_rel, n_chains, n_hdr, 0u, pat_fold, tests, n_relative, reach, msg);
}

int kmp_pack_bytetests(const kmpgpu_bytetest *bt, uint32_t n_bt, uint32_t n_pat, uint32_t n_rel, uint32_t n_chains, uint32_t n_hdr,
                       uint32_t n_rx, const uint8_t *pat_fold, std::vector<uint32_t> *tests, uint32_t *n_relative, uint32_t *reach,
                       std::string *msg)
{
    tests->clear();
    *n_relative = 0u; *reach = 0u;
    if (!bt) return refuse(msg, "kmpgpu_set_bytetests: bt is NULL");
    if ((uint64_t)n_pat + n_rel + n_chains + n_hdr + n_bt + n_rx >= (1ull << 31))
        return refuse(msg, "kmpgpu_set_bytetests: %u patterns + %u relations + %u chains + %u header predicates + %u byte tests%s do not fit the 2^31 rows a rule term can name",
                      n_pat, n_rel, n_chains, n_hdr, n_bt, n_rx ? " + the expressions" : "");
    std::vector<uint32_t> recs, relative;             /* a refusal leaves *tests empty */
    uint32_t far = 0u;
    for (uint32_t q = 0; q < n_bt; q++) {
        const kmpgpu_bytetest &b = bt[q];
        if (b.nbytes < 1 || b.nbytes > 4) return refuse(msg, "kmpgpu_set_bytetests: test %u reads %u bytes, not 1 .. 4", q, b.nbytes);
        if (b.op > KMPGPU_BT_GE) return refuse(msg, "kmpgpu_set_bytetests: test %u: unknown operator %u", q, b.op);
        if (b.flags & ~(KMPGPU_BT_RELATIVE | KMPGPU_BT_LITTLE))
            return refuse(msg, "kmpgpu_set_bytetests: test %u: unknown flag bits 0x%x", q, b.flags & ~(KMPGPU_BT_RELATIVE | KMPGPU_BT_LITTLE));
        if (b.reserved != 0) return refuse(msg, "kmpgpu_set_bytetests: test %u: reserved is %u, not 0", q, b.reserved);
        uint32_t anchor = 0u;
        if (b.flags & KMPGPU_BT_RELATIVE) {
            if (b.anchor >= n_pat) return refuse(msg, "kmpgpu_set_bytetests: test %u names pattern %u of %u", q, b.anchor, n_pat);
            anchor = fold_bit(pat_fold, b.anchor);
            relative.push_back(q);
        } else {
            if (b.anchor != 0) return refuse(msg, "kmpgpu_set_bytetests: test %u is absolute and names anchor %u, not 0", q, b.anchor);
            if (b.offset < 0) return refuse(msg, "kmpgpu_set_bytetests: test %u is absolute and its offset %d lies in front of the payload", q, b.offset);
            if ((uint32_t)b.offset + b.nbytes > far) far = (uint32_t)b.offset + b.nbytes;
        }
        recs.insert(recs.end(), {anchor, (uint32_t)b.offset, b.mask, b.value,
                                     (uint32_t)b.nbytes | (uint32_t)b.op << 8 | (uint32_t)b.flags << 16, 0u, 0u, 0u});
    }
    *n_relative = (uint32_t)relative.size();
    *reach = far;
    tests->swap(recs);
    tests->insert(tests->end(), relative.begin(), relative.end());
    return KMPGPU_OK;
}

int kmp_pack_flowbits(const kmpgpu_flowbit_op *ops, uint32_t n_ops, uint32_t n_bits, uint32_t n_rules, kmp_flowbit_tables *out,
                      std::string *msg)
{
    *out = kmp_flowbit_tables{};
    if (n_bits < 1u || n_bits > KMPGPU_FLOWBITS_MAX)
        return refuse(msg, "kmpgpu_set_flowbits: n_bits is %u, outside 1..%u", n_bits, (unsigned)KMPGPU_FLOWBITS_MAX);
    if (!ops) return refuse(msg, "kmpgpu_set_flowbits: ops is NULL");
    for (uint32_t j = 0; j < n_ops; j++) {
        const kmpgpu_flowbit_op &o = ops[j];
        if (o.rule >= n_rules) return refuse(msg, "kmpgpu_set_flowbits: op %u names rule %u of %u", j, o.rule, n_rules);
        if (o.op > KMPGPU_FB_NOALERT) return refuse(msg, "kmpgpu_set_flowbits: op %u: %u is none of KMPGPU_FB_*", j, o.op);
        if (o.reserved) return refuse(msg, "kmpgpu_set_flowbits: op %u: the reserved field is %u, not 0", j, o.reserved);
        if (o.op != KMPGPU_FB_NOALERT && o.bit >= n_bits) return refuse(msg, "kmpgpu_set_flowbits: op %u names bit %u of %u", j, o.bit, n_bits);
    }
    /* per rule: what it tests, what it acts on */
    std::vector<uint32_t> isset(n_rules, 0u), isnotset(n_rules, 0u), acts(n_rules, 0u), noalert(n_rules, 0u);
    for (uint32_t j = 0; j < n_ops; j++) {
        const kmpgpu_flowbit_op &o = ops[j];
        const uint32_t b = o.op == KMPGPU_FB_NOALERT ? 0u : 1u << o.bit;
        if (o.op == KMPGPU_FB_ISSET) isset[o.rule] |= b;
        else if (o.op == KMPGPU_FB_ISNOTSET) isnotset[o.rule] |= b;
        else if (o.op == KMPGPU_FB_NOALERT) noalert[o.rule] = 1u;
        else acts[o.rule] |= b;
        if (isset[o.rule] & isnotset[o.rule])
            return refuse(msg, "kmpgpu_set_flowbits: op %u: rule %u tests bit %u both set and clear", j, o.rule, o.bit);
    }
    /* succ[Y]: the bits X != Y that a rule testing Y acts on */
    uint32_t succ[KMPGPU_FLOWBITS_MAX] = {0};
    for (uint32_t r = 0; r < n_rules; r++)
        for (uint32_t y = 0; y < n_bits; y++)
            if ((isset[r] | isnotset[r]) >> y & 1u) succ[y] |= acts[r] & ~(1u << y);
    /* longest paths by relaxation: without a cycle no level passes n_bits - 1 */
    out->level_of.assign(n_bits, 0u);
    bool moved = true;
    for (uint32_t round = 0; moved && round <= n_bits; round++) {
        moved = false;
        for (uint32_t y = 0; y < n_bits; y++)
            for (uint32_t x = 0; x < n_bits; x++)
                if ((succ[y] >> x & 1u) && out->level_of[x] < out->level_of[y] + 1u) { out->level_of[x] = out->level_of[y] + 1u; moved = true; }
    }
    if (moved) {
        /* depth first from every bit, the path kept: an edge back into the path closes a cycle, named from the lowest start that finds one */
        std::string path;
        uint32_t done = 0;
        for (uint32_t s = 0; s < n_bits && path.empty(); s++) {
            uint32_t stack[KMPGPU_FLOWBITS_MAX], next[KMPGPU_FLOWBITS_MAX], depth = 0, on = 0;
            if (done >> s & 1u) continue;
            stack[0] = s; next[0] = 0; on = 1u << s; depth = 1;
            while (depth && path.empty()) {
                const uint32_t v = stack[depth - 1];
                uint32_t x = next[depth - 1];
                while (x < n_bits && (!(succ[v] >> x & 1u) || (done >> x & 1u))) x++;
                next[depth - 1] = x + 1u;
                if (x >= n_bits) { done |= 1u << v; on &= ~(1u << v); depth--; continue; }
                if (on >> x & 1u) {
                    uint32_t i = 0;
                    while (stack[i] != x) i++;
                    for (; i < depth; i++) path += std::to_string(stack[i]) + " -> ";
                    path += std::to_string(x);
                } else { stack[depth] = x; next[depth] = 0; on |= 1u << x; depth++; }
            }
        }
        *out = kmp_flowbit_tables{};
        return refuse(msg, "kmpgpu_set_flowbits: the flow bits %s form a cycle (a rule tests one and acts on the next)", path.c_str());
    }
    out->n_bits = n_bits;
    for (uint32_t b = 0; b < n_bits; b++) out->n_levels = out->level_of[b] + 1u > out->n_levels ? out->level_of[b] + 1u : out->n_levels;
    out->level_mask.assign(out->n_levels, 0u);
    for (uint32_t b = 0; b < n_bits; b++) out->level_mask[out->level_of[b]] |= 1u << b;
    uint32_t lower = 0;
    for (uint32_t l = 0; l < out->n_levels; l++) {
        const uint32_t lm = out->level_mask[l];
        out->level_first.push_back((uint32_t)(out->acting.size() / 8u));
        for (uint32_t r = 0; r < n_rules; r++) {
            if (!(acts[r] & lm)) continue;
            uint32_t a0 = 0u, a1 = ~0u;
            for (uint32_t j = 0; j < n_ops; j++) {
                const kmpgpu_flowbit_op &o = ops[j];
                if (o.rule != r || o.op < KMPGPU_FB_SET || o.op > KMPGPU_FB_TOGGLE || !(lm >> o.bit & 1u)) continue;
                const uint32_t b = 1u << o.bit;
                if (o.op == KMPGPU_FB_SET) { a0 |= b; a1 |= b; }
                else if (o.op == KMPGPU_FB_UNSET) { a0 &= ~b; a1 &= ~b; }
                else { a0 ^= b; a1 ^= b; }
            }
            const uint32_t self = ((isset[r] & lm) ? 1u : 0u) | ((isnotset[r] & lm) ? 2u : 0u);
            out->acting.insert(out->acting.end(), {r, isset[r] & lower, isnotset[r] & lower, self, a0, a1, 0u, 0u});
        }
        lower |= lm;
    }
    out->level_first.push_back((uint32_t)(out->acting.size() / 8u));
    for (uint32_t r = 0; r < n_rules; r++) out->tests.insert(out->tests.end(), {isset[r], isnotset[r], noalert[r], 0u});
    return KMPGPU_OK;
}

int kmp_pack_thresholds(const kmpgpu_threshold *thr, uint32_t n_thr, uint32_t n_rules, kmp_threshold_tables *out, std::string *msg)
{
    *out = kmp_threshold_tables{};
    if (!thr) return refuse(msg, "kmpgpu_set_thresholds: thr is NULL");
    for (uint32_t q = 0; q < n_thr; q++) {
        const kmpgpu_threshold &t = thr[q];
        if (t.rule >= n_rules) return refuse(msg, "kmpgpu_set_thresholds: threshold %u names rule %u of %u", q, t.rule, n_rules);
        if (t.track > KMPGPU_THR_BY_FLOW) return refuse(msg, "kmpgpu_set_thresholds: threshold %u: track %u is none of KMPGPU_THR_BY_*", q, t.track);
        if (t.type > KMPGPU_THR_EXACTLY) return refuse(msg, "kmpgpu_set_thresholds: threshold %u: type %u is none of KMPGPU_THR_AT_LEAST, _AT_MOST, _EXACTLY", q, t.type);
        if (t.count == 0) return refuse(msg, "kmpgpu_set_thresholds: threshold %u: count is 0", q);
        if (t.window == 0) return refuse(msg, "kmpgpu_set_thresholds: threshold %u: window is 0 (no payload lies inside it)", q);
    }
    for (uint32_t q = 0; q < n_thr; q++) {
        out->by_track[thr[q].track].push_back(q);
        if (thr[q].window != KMPGPU_THR_NO_WINDOW) out->windowed = true;
    }
    /* {first, number} per rule, then the rules' thresholds rule by rule, each rule's in the order given */
    out->final_table.assign(2u * (size_t)n_rules, 0u);
    for (uint32_t q = 0; q < n_thr; q++) out->final_table[2u * (size_t)thr[q].rule + 1u]++;
    uint32_t first = 0;
    for (uint32_t r = 0; r < n_rules; r++) { out->final_table[2u * (size_t)r] = first; first += out->final_table[2u * (size_t)r + 1u]; }
    std::vector<uint32_t> fill(n_rules, 0u);
    out->final_table.resize(2u * (size_t)n_rules + n_thr, 0u);
    for (uint32_t q = 0; q < n_thr; q++) {
        const uint32_t r = thr[q].rule;
        out->final_table[2u * (size_t)n_rules + out->final_table[2u * (size_t)r] + fill[r]++] = q;
    }
    return KMPGPU_OK;
}
