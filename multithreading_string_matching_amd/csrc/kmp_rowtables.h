/*
 * kmp_rowtables.h -- what kmpgpu_set_rules, kmpgpu_set_windows, kmpgpu_set_relations, kmpgpu_set_chains, kmpgpu_set_headers, kmpgpu_set_bytetests, kmpgpu_set_regexes, kmpgpu_set_flowbits and kmpgpu_set_thresholds upload, checked and packed on
 * the host by kmp_rowtables.cpp into the form the kernels read bit for bit (kmp_launch.h: kmp_launch_rules, emit_windows,
 * kmp_launch_relations, kmp_launch_chains, kmp_launch_headers, kmp_launch_bytetests, kmp_launch_regexes).  Host code without a HIP header, as kmp_tables.h: it builds and runs without a device
 * (tests/rowtables_sanitizer_driver.cpp).
 *
 * Every packer returns KMPGPU_OK with its table -- 16-byte records as four uint32_t, window records as two -- or KMPGPU_EINVAL with the
 * whole text of kmpgpu_last_error in *msg.  It reads none of its arrays before the counts alone have passed.  n_pat, n_rel, n_chains, n_hdr:
 * the rows of the context's hit matrix (the entries without n_hdr are the ones with n_hdr = 0); pat_fold[i]: pattern i is compared in the folded copy of the arena (bit 31 of its index in a record).
 */
#ifndef KMP_ROWTABLES_H
#define KMP_ROWTABLES_H

#include <stdint.h>

#include <string>
#include <vector>

#include "kmpgpu.h"

/* heads[r] = {first quad of rule r's further terms, the quad behind its last, first term, second term}, quads[q] = four further terms: a
 * rule's plain terms in front of its negated ones (a lane of the kernel whose payloads miss one of them stops early), a rule of one term
 * with it twice in its head, the last quad filled up with repeats of its own first term. */
int kmp_pack_rules(const uint32_t *rule_off, const uint32_t *terms, uint32_t n_rules, uint32_t n_pat, uint32_t n_rel, uint32_t n_chains,
                   std::vector<uint32_t> *heads, std::vector<uint32_t> *quads, std::string *msg);

/* {first, last} per pattern; empty where every window is the default [0, UINT32_MAX]: no table, the emitting passes run as without */
int kmp_pack_windows(const uint32_t *first, const uint32_t *last, uint32_t n_windows, uint32_t n_pat, std::vector<uint32_t> *windows,
                     std::string *msg);

/* {a | fold << 31, b | fold << 31, dmin, dmax} per relation */
int kmp_pack_relations(const kmpgpu_relation *rel, uint32_t n_rel, uint32_t n_pat, uint32_t n_chains, const uint8_t *pat_fold,
                       std::vector<uint32_t> *relations, std::string *msg);

/* KMPGPU_CHAIN_MAX records {pattern | fold << 31, dmin, dmax, n} per chain of n contents, the records behind the last link repeating it */
int kmp_pack_chains(const uint32_t *chain_off, const kmpgpu_chain_link *links, uint32_t n_chains, uint32_t n_pat, uint32_t n_rel,
                    const uint8_t *pat_fold, std::vector<uint32_t> *chains, std::string *msg);

/* The same with the header predicates' rows behind the chains': a rule's terms name rows below n_pat + n_rel + n_chains + n_hdr, and the
 * 2^31 bound of the relations and chains counts them in. */
int kmp_pack_rules(const uint32_t *rule_off, const uint32_t *terms, uint32_t n_rules, uint32_t n_pat, uint32_t n_rel, uint32_t n_chains,
                   uint32_t n_hdr, std::vector<uint32_t> *heads, std::vector<uint32_t> *quads, std::string *msg);
int kmp_pack_relations(const kmpgpu_relation *rel, uint32_t n_rel, uint32_t n_pat, uint32_t n_chains, uint32_t n_hdr, const uint8_t *pat_fold,
                       std::vector<uint32_t> *relations, std::string *msg);
int kmp_pack_chains(const uint32_t *chain_off, const kmpgpu_chain_link *links, uint32_t n_chains, uint32_t n_pat, uint32_t n_rel,
                    uint32_t n_hdr, const uint8_t *pat_fold, std::vector<uint32_t> *chains, std::string *msg);

/* Three 16-byte records per predicate: {src_ip & src_mask, src_mask, dst_ip & dst_mask, dst_mask}, {sport_lo | sport_hi << 16,
 * dport_lo | dport_hi << 16, len_lo, len_hi}, {proto | flags << 8, 0, 0, 0} */
int kmp_pack_headers(const kmpgpu_header *h, uint32_t n_hdr, uint32_t n_pat, uint32_t n_rel, uint32_t n_chains, std::vector<uint32_t> *headers,
                     std::string *msg);

/* The same once more with the byte tests' rows behind the header predicates': terms name rows below n_pat + n_rel + n_chains + n_hdr + n_bt,
 * and every 2^31 bound counts n_bt in.  With n_bt = 0 every message is what the entries above give. */
int kmp_pack_rules(const uint32_t *rule_off, const uint32_t *terms, uint32_t n_rules, uint32_t n_pat, uint32_t n_rel, uint32_t n_chains,
                   uint32_t n_hdr, uint32_t n_bt, std::vector<uint32_t> *heads, std::vector<uint32_t> *quads, std::string *msg);
int kmp_pack_relations(const kmpgpu_relation *rel, uint32_t n_rel, uint32_t n_pat, uint32_t n_chains, uint32_t n_hdr, uint32_t n_bt,
                       const uint8_t *pat_fold, std::vector<uint32_t> *relations, std::string *msg);
int kmp_pack_chains(const uint32_t *chain_off, const kmpgpu_chain_link *links, uint32_t n_chains, uint32_t n_pat, uint32_t n_rel,
                    uint32_t n_hdr, uint32_t n_bt, const uint8_t *pat_fold, std::vector<uint32_t> *chains, std::string *msg);
int kmp_pack_headers(const kmpgpu_header *h, uint32_t n_hdr, uint32_t n_pat, uint32_t n_rel, uint32_t n_chains, uint32_t n_bt,
                     std::vector<uint32_t> *headers, std::string *msg);

/* Two 16-byte records per test: {anchor | fold << 31 (0 for an absolute test), offset, mask, value}, {nbytes | op << 8 | flags << 16, 0, 0, 0};
 * behind the 8 n_bt words of the records the *n_relative indices of the relative tests, ascending (the relative kernel's work list).
 * *reach: the largest offset + nbytes of the absolute tests, 0 without one (H of kmp_launch_bytetests). */
int kmp_pack_bytetests(const kmpgpu_bytetest *bt, uint32_t n_bt, uint32_t n_pat, uint32_t n_rel, uint32_t n_chains, uint32_t n_hdr,
                       const uint8_t *pat_fold, std::vector<uint32_t> *tests, uint32_t *n_relative, uint32_t *reach, std::string *msg);

/* The same once more with the expressions' rows behind the byte tests' (kmpgpu_set_regexes): terms name rows below
 * n_pat + n_rel + n_chains + n_hdr + n_bt + n_rx, and every 2^31 bound counts n_rx in.  With n_rx = 0 every message is what the entries
 * above give. */
int kmp_pack_rules(const uint32_t *rule_off, const uint32_t *terms, uint32_t n_rules, uint32_t n_pat, uint32_t n_rel, uint32_t n_chains,
                   uint32_t n_hdr, uint32_t n_bt, uint32_t n_rx, std::vector<uint32_t> *heads, std::vector<uint32_t> *quads, std::string *msg);
int kmp_pack_relations(const kmpgpu_relation *rel, uint32_t n_rel, uint32_t n_pat, uint32_t n_chains, uint32_t n_hdr, uint32_t n_bt,
                       uint32_t n_rx, const uint8_t *pat_fold, std::vector<uint32_t> *relations, std::string *msg);
int kmp_pack_chains(const uint32_t *chain_off, const kmpgpu_chain_link *links, uint32_t n_chains, uint32_t n_pat, uint32_t n_rel,
                    uint32_t n_hdr, uint32_t n_bt, uint32_t n_rx, const uint8_t *pat_fold, std::vector<uint32_t> *chains, std::string *msg);
int kmp_pack_headers(const kmpgpu_header *h, uint32_t n_hdr, uint32_t n_pat, uint32_t n_rel, uint32_t n_chains, uint32_t n_bt, uint32_t n_rx,
                     std::vector<uint32_t> *headers, std::string *msg);
int kmp_pack_bytetests(const kmpgpu_bytetest *bt, uint32_t n_bt, uint32_t n_pat, uint32_t n_rel, uint32_t n_chains, uint32_t n_hdr,
                       uint32_t n_rx, const uint8_t *pat_fold, std::vector<uint32_t> *tests, uint32_t *n_relative, uint32_t *reach,
                       std::string *msg);

/* The same once more with the links' rows behind the expressions' (kmpgpu_set_links): terms name rows below
 * n_pat + n_rel + n_chains + n_hdr + n_bt + n_rx + n_links.  The links have no table of their own, so the other packers do not know them;
 * kmpgpu_set_links holds the sum below 2^31.  With n_links = 0 every message is what the entries above give. */
int kmp_pack_rules(const uint32_t *rule_off, const uint32_t *terms, uint32_t n_rules, uint32_t n_pat, uint32_t n_rel, uint32_t n_chains,
                   uint32_t n_hdr, uint32_t n_bt, uint32_t n_rx, uint32_t n_links, std::vector<uint32_t> *heads, std::vector<uint32_t> *quads,
                   std::string *msg);

/* (defined in kmp_regex.cpp, beside the compiler it calls: kmp_rowtables.cpp links without it)  The expressions compiled (kmp_regex.h:
 * kmp_regex_compile) and laid out in tiles of KMP_RX_TILE as kmp_regex.h describes the device table;
 * ceil(n_rx / KMP_RX_TILE) * KMP_RX_TILE_WORDS words.  flags NULL: all 0; gate NULL: none gated.  An unknown flag bit, a gate >= n_pat of
 * a gated expression, a gate != 0 of one that is not, an expression outside the dialect ("expression Q: position P: ..."): KMPGPU_EINVAL.
 * An expression under KMPGPU_RX_GROUPS is checked here too (kmp_regex_compile_groups), so this one call refuses a bad set; its slot holds a
 * placeholder -- one position that no byte takes, gated on the expression's own row n_pat + n_rel + n_chains + n_hdr + n_bt + q, which the
 * marking pass has zeroed: no lane is active for it and the linear kernel stores zeros there.  A set without the flag packs as it did. */
int kmp_pack_regexes(const uint8_t *const *expr, const uint32_t *expr_len, const uint32_t *flags, const uint32_t *gate, uint32_t n_rx,
                     uint32_t n_pat, uint32_t n_rel, uint32_t n_chains, uint32_t n_hdr, uint32_t n_bt, std::vector<uint32_t> *tables,
                     std::string *msg);

/* (kmp_regex.cpp too)  The second device table: the expressions under KMPGPU_RX_GROUPS alone, in their order, in tiles of KMP_RXG_TILE as
 * kmp_regex.h describes them, each record carrying its expression's index q; ceil(*n_groups / KMP_RXG_TILE) * KMP_RXG_TILE_WORDS words,
 * none where no expression carries the flag.  The same checks and messages as kmp_pack_regexes. */
int kmp_pack_regex_groups(const uint8_t *const *expr, const uint32_t *expr_len, const uint32_t *flags, const uint32_t *gate, uint32_t n_rx,
                          uint32_t n_pat, uint32_t n_rel, uint32_t n_chains, uint32_t n_hdr, uint32_t n_bt, std::vector<uint32_t> *tables,
                          uint32_t *n_groups, std::string *msg);

/* kmpgpu_set_flowbits: the ops checked, the bits' levels, and the two tables the kernels of kmp_flowbits.hip read (kmp_launch.h).
 * level_of[n_bits]: the longest path into the bit in the graph with an edge Y -> X where a rule tests Y and acts on X != Y (a self-loop is
 * no edge); level_mask[n_levels]: the bits of a level; level_first[n_levels + 1]: the level's records in `acting`.
 * acting: 8 words per (level, rule that acts on a bit of the level), the rules of a level in ascending index: {rule, the bits of lower
 * levels it tests set, those it tests clear, self, a0, a1, 0, 0}.  self: bit 0 -- it tests a bit of this level set (by the graph that is the
 * one bit of the level it acts on), bit 1 -- clear.  (a0, a1): its actions on the level's bits, in the order given, composed into one
 * function per bit -- bit X of a0 is what they make of X = 0, of a1 of X = 1; identity (0, 1) for every other bit.
 * tests: 4 words per rule: {bits tested set, bits tested clear, 1 for a NOALERT rule, 0}.
 * Refusals (KMPGPU_EINVAL, the text of kmpgpu_last_error in *msg): n_bits outside 1..KMPGPU_FLOWBITS_MAX, ops NULL, a rule >= n_rules, a
 * bit >= n_bits (not looked at for NOALERT), an unknown op, a nonzero reserved field, a (rule, bit) tested both ways, a cycle. */
struct kmp_flowbit_tables {
    uint32_t n_bits = 0, n_levels = 0;
    std::vector<uint32_t> level_of, level_mask, level_first, acting, tests;
};
int kmp_pack_flowbits(const kmpgpu_flowbit_op *ops, uint32_t n_ops, uint32_t n_bits, uint32_t n_rules, kmp_flowbit_tables *out,
                      std::string *msg);

/* kmpgpu_set_thresholds: the thresholds checked and grouped.  by_track[KMPGPU_THR_BY_*]: the indices q of the track's thresholds in
 * ascending order -- what the C-ABI layer walks: one order per track in use, then the track's thresholds; windowed: some window is not
 * KMPGPU_THR_NO_WINDOW (the timestamps are needed).  final_table, what kmp_thresholds.hip's final kernel reads: two words per rule {first,
 * number} into the list behind them [n_thr], which holds the indices q (the pass rows) of every rule's thresholds, rule by rule, each
 * rule's in the order given.
 * Refusals (KMPGPU_EINVAL, the text of kmpgpu_last_error in *msg): thr NULL, a rule >= n_rules, an unknown track or type, count == 0,
 * window == 0. */
struct kmp_threshold_tables {
    std::vector<uint32_t> by_track[4], final_table;
    bool windowed = false;
};
int kmp_pack_thresholds(const kmpgpu_threshold *thr, uint32_t n_thr, uint32_t n_rules, kmp_threshold_tables *out, std::string *msg);

#endif
