/*
 * kmp_tables.h -- what kmpgpu_set_patterns uploads for one set of patterns, built on the host by kmp_tables.cpp: the id order of
 * the streaming passes and the table blobs of the fused multi-pattern pass (layout: kmp_device.h, read bit for bit by
 * kmp_scan_multi.hip).  Host code without a HIP header: it builds and runs without a device (tests/tables_sanitizer_driver.cpp).
 */
#ifndef KMP_TABLES_H
#define KMP_TABLES_H

#include <stdint.h>

#include <vector>

#include "kmp_device.h"

/* one group of the fused pass: at most KMP_MULTI_MAX_UNIQUE distinct patterns, a classed group four times as many */
struct kmp_group_tables {
    std::vector<uint32_t> tables;               /* layout: kmp_device.h KMP_MULTI_*                                  */
    std::vector<uint32_t> ids, rows;            /* the pattern indices this group counts and the row of each         */
    std::vector<uint32_t> uid_first, uid_ids;   /* row -> pattern indices (offset emission): CSR, n_unique + 1 firsts */
    uint32_t n_unique = 0;                      /* rows: the distinct patterns, then the 1-byte patterns riding along */
    uint32_t cshift = 0;                        /* a plain group's short patterns, a classed one's class shift       */
    uint32_t bmask = 0, n_ones = 0, ones = 0;
    bool     classed = false;
};

struct kmp_set_tables {
    std::vector<uint32_t> ids;                  /* every member: long patterns (m >= 4) first, then short            */
    uint32_t n_long = 0, n_short = 0;
    std::vector<kmp_group_tables> groups;       /* empty: nothing to fuse, every pattern keeps its own pass (ids)    */
    uint32_t n_multi_unique = 0;                /* distinct eligible patterns over all groups                        */
    std::vector<uint32_t> rest;                 /* with groups: the members no group counts, long first              */
    uint32_t rest_long = 0, rest_short = 0;
};

/* The passes of one set over the patterns `members` (indices into host, file order), built on the bytes as stored (folded for the
 * nocase set, so that "HOST" and "Host" share a row).  false: a group's entry list overflowed. */
bool kmp_build_tables(const kmp_pattern_dev *host, const std::vector<uint32_t> &members, kmp_set_tables *out);

#endif
