/*
 * kmp_tables.cpp -- the tables kmpgpu_set_patterns uploads for one set of patterns (kmp_tables.h).  Host code only.
 */
#include "kmp_tables.h"

#include <algorithm>
#include <string>
#include <unordered_map>
#include <utility>

bool kmp_build_tables(const kmp_pattern_dev *host, const std::vector<uint32_t> &members, kmp_set_tables *out)
{
    kmp_set_tables &s = *out;
    s = kmp_set_tables{};
    for (const uint32_t i : members) if (host[i].m >= 4) s.ids.push_back(i);
    s.n_long = (uint32_t)s.ids.size();
    for (const uint32_t i : members) if (host[i].m < 4) s.ids.push_back(i);
    s.n_short = (uint32_t)members.size() - s.n_long;

    /* ---- tables of the fused multi-pattern pass (layout: kmp_device.h) ------------------------- */
    /* a group: its distinct patterns, the row (unique-pattern id of the kernel) of each, the patterns counted by it and their rows.
     * `classed`: more than 256 rows -- an entry has eight bits for an id, the kernel adds the first id of the bucket's class
     * (= bucket >> 7: eight classes of up to 256 patterns each, 1024 in all; kmp_device.h) */
    constexpr uint32_t NCLS = KMP_MULTI_CLS_WORDS;
    struct HostGroup { std::vector<std::string> uniq; std::vector<uint32_t> gidx, row; std::vector<uint32_t> ids, rows; bool classed = false;
                       uint32_t n_cls[NCLS] = {}, overflow = 0; std::vector<uint8_t> bucket_used; };
    std::vector<HostGroup> hg;
    std::vector<uint32_t> rest_l, rest_s;
    /* 1-byte patterns: up to KMP_MULTI_MAX_ONES distinct ones ride along with the first fused group (counted straight
     * off the text registers, no filter, no queue); further ones keep one streaming pass each */
    std::vector<uint8_t> one_bytes;
    std::vector<std::pair<uint32_t, uint32_t>> one_ids;            /* (pattern index, slot) */
    std::vector<std::string> uniq_all;                             /* the distinct eligible patterns, file order */
    std::vector<uint32_t> first_pat;                               /* ... and the first pattern of the list that is each of them */
    std::unordered_map<std::string, uint32_t> uniq_of;
    std::vector<std::pair<uint32_t, uint32_t>> elig;               /* (pattern index, its distinct pattern) */
    for (const uint32_t i : members) {
        const uint8_t *const pi = host[i].pat;
        const uint32_t m = host[i].m;
        if (m == 1) {
            size_t k = 0;
            while (k < one_bytes.size() && one_bytes[k] != pi[0]) k++;
            if (k == one_bytes.size() && k < KMP_MULTI_MAX_ONES) one_bytes.push_back(pi[0]);
            if (k < one_bytes.size()) { one_ids.emplace_back(i, (uint32_t)k); continue; }
        }
        if (m < KMP_MULTI_MIN_LEN || m > KMP_MULTI_MAX_LEN) { (m >= 4 ? rest_l : rest_s).push_back(i); continue; }
        const std::string key((const char *)pi, m);
        auto it = uniq_of.find(key);
        if (it == uniq_of.end()) {
            /* (a record names the pattern whose bytes 8 .. m-1 the kernel compares against in 16 bits: a pattern of nine bytes or
             * more that first occurs behind the 65 536th of the list keeps a pass of its own) */
            if (m > 8 && i > 0xFFFFu) { rest_l.push_back(i); continue; }
            it = uniq_of.emplace(key, (uint32_t)uniq_all.size()).first; uniq_all.push_back(key); first_pat.push_back(i);
        }
        elig.emplace_back(i, it->second);
    }
    if (uniq_all.size() < 2) {                    /* nothing to fuse: every pattern keeps its own pass (ids) */
        return true;
    }
    /* Which group a distinct pattern goes to.  Up to 256 of them: one group, rows in file order (short ones first, below).  More: the
     * 2-byte patterns (entered under every third byte: 32 buckets each, in all classes) and, if 1-byte patterns ride along, the first
     * patterns of the file fill plain groups of 256; everything else goes to classed groups of up to 1024 -- first fit, a pattern
     * whose class is full (256) or whose bucket would overflow the entry list waits for the next group. */
    std::vector<std::pair<uint32_t, uint32_t>> place(uniq_all.size());        /* distinct pattern -> (group, index in its uniq) */
    auto key_class = [](const std::string &p) {
        const uint32_t w24 = (uint8_t)p[0] | ((uint32_t)(uint8_t)p[1] << 8) | ((uint32_t)(uint8_t)p[2] << 16);
        return KMP_MULTI_HASH(w24 & KMP_MULTI_KEYMASK);
    };
    {
        const bool big = uniq_all.size() > KMP_MULTI_MAX_UNIQUE;
        std::vector<uint32_t> plain, classed;
        for (uint32_t u = 0; u < uniq_all.size(); u++) (!big || uniq_all[u].size() == 2 ? plain : classed).push_back(u);
        if (big && plain.empty() && !one_bytes.empty()) {                     /* the 1-byte patterns need a plain first group */
            const size_t take = std::min<size_t>(classed.size(), KMP_MULTI_MAX_UNIQUE);
            plain.assign(classed.begin(), classed.begin() + take);
            classed.erase(classed.begin(), classed.begin() + take);
        }
        for (uint32_t u : plain) {
            if (hg.empty() || hg.back().uniq.size() == KMP_MULTI_MAX_UNIQUE) hg.emplace_back();
            place[u] = {(uint32_t)hg.size() - 1u, (uint32_t)hg.back().uniq.size()};
            hg.back().uniq.push_back(uniq_all[u]); hg.back().gidx.push_back(u);
        }
        const size_t first_classed = hg.size();
        for (uint32_t u : classed) {
            const std::string &p = uniq_all[u];
            const uint32_t b = key_class(p), cl = b >> KMP_MULTI_CLS_SHIFT;
            size_t gi = first_classed;
            for (; gi < hg.size(); gi++) {
                HostGroup &h = hg[gi];
                if (h.uniq.size() < 4u * KMP_MULTI_MAX_UNIQUE && h.n_cls[cl] < 256u && h.overflow + (h.bucket_used[b] ? 1u : 0u) <= KMP_MULTI_MAX_ENTRIES) break;
            }
            if (gi == hg.size()) { hg.emplace_back(); hg.back().classed = true; hg.back().bucket_used.assign(KMP_MULTI_BUCKETS, 0); }
            HostGroup &h = hg[gi];
            h.n_cls[cl]++;
            if (h.bucket_used[b]) h.overflow++; else h.bucket_used[b] = 1;
            place[u] = {(uint32_t)gi, (uint32_t)h.uniq.size()};
            h.uniq.push_back(p); h.gidx.push_back(u);
        }
    }
    bool first_group = true;
    for (HostGroup &h : hg) {
        const uint32_t U = (uint32_t)h.uniq.size();
        const uint32_t n_ones = first_group ? (uint32_t)one_bytes.size() : 0u;
        uint32_t ones = 0;
        for (uint32_t k = 0; k < n_ones; k++) ones |= (uint32_t)one_bytes[k] << (8 * k);
        first_group = false;
        /* rows: class by class, short patterns (2 or 3 bytes: decided by their bucket entry alone) first in each (a plain group is one class) */
        uint32_t cls_short[NCLS] = {}, cls_n[NCLS] = {}, rec_base[NCLS] = {}, row_base[NCLS] = {};
        std::vector<uint32_t> cls_of(U, 0u), in_cls(U, 0u);
        h.row.assign(U, 0u);
        for (uint32_t u = 0; u < U; u++) {
            cls_of[u] = h.classed ? key_class(h.uniq[u]) >> KMP_MULTI_CLS_SHIFT : 0u;
            cls_n[cls_of[u]]++;
            if (h.uniq[u].size() <= KMP_MULTI_SHORT_LEN) cls_short[cls_of[u]]++;
        }
        for (uint32_t cl = 1; cl < NCLS; cl++) {
            row_base[cl] = row_base[cl - 1] + cls_n[cl - 1];
            rec_base[cl] = rec_base[cl - 1] + (cls_n[cl - 1] - cls_short[cl - 1]);
        }
        {
            uint32_t next_short[NCLS] = {}, next_long[NCLS];
            for (uint32_t cl = 0; cl < NCLS; cl++) next_long[cl] = cls_short[cl];
            for (uint32_t u = 0; u < U; u++) {
                const uint32_t cl = cls_of[u];
                in_cls[u] = h.uniq[u].size() <= KMP_MULTI_SHORT_LEN ? next_short[cl]++ : next_long[cl]++;
                h.row[u] = row_base[cl] + in_cls[u];
            }
        }
        const uint32_t rows_n = U;
        const uint32_t n_long = rec_base[NCLS - 1] + (cls_n[NCLS - 1] - cls_short[NCLS - 1]);
        std::vector<uint32_t> tab(KMP_MULTI_REC_W0 + (h.classed ? KMP_MULTI_CLS_WORDS + (size_t)n_long * KMP_MULTI_CREC_WORDS : (size_t)n_long * KMP_MULTI_REC_WORDS), 0u);
        if (h.classed)
            for (uint32_t cl = 0; cl < NCLS; cl++) tab[KMP_MULTI_REC_W0 + cl] = KMP_MULTI_CLS_WORD(cls_short[cl], rec_base[cl], row_base[cl]);
        uint32_t *bucket = tab.data() + KMP_MULTI_BUCKET_W0;
        uint32_t *entry = tab.data() + KMP_MULTI_ENTRY_W0;
        std::vector<std::vector<uint32_t>> lists(KMP_MULTI_BUCKETS);
        uint32_t n_two = 0;
        for (uint32_t u = 0; u < U; u++) n_two += h.uniq[u].size() == 2 ? 1u : 0u;
        const uint32_t bmask = n_two <= KMP_MULTI_MAX_TWO ? KMP_MULTI_KEYMASK : 0xFFFFu;        /* bucket key: three bytes, or two when 2-byte patterns abound */
        for (uint32_t u = 0; u < U; u++) {
            const std::string &p = h.uniq[u];
            const uint32_t w16 = (uint8_t)p[0] | ((uint32_t)(uint8_t)p[1] << 8);
            uint32_t *pair = tab.data() + KMP_MULTI_FILTER_W0;
            if (p.size() >= 3) {
                pair[2u * KMP_MULTI_PAIR(p[1], p[2])]      |= 1u << ((uint8_t)p[0] & 31u);       /* p0 may stand before p1 p2 */
                pair[2u * KMP_MULTI_PAIR(p[0], p[1]) + 1u] |= 1u << ((uint8_t)p[2] & 31u);       /* p2 may follow p0 p1       */
            } else {
                for (uint32_t t = 0; t < 32u; t++) pair[2u * KMP_MULTI_PAIR(p[1], t)] |= 1u << ((uint8_t)p[0] & 31u);
                pair[2u * KMP_MULTI_PAIR(p[0], p[1]) + 1u] = 0xFFFFFFFFu;                       /* whatever follows        */
            }
            for (uint32_t t = 0; t < 32u; t++) {                      /* a 2-byte pattern matches whatever follows it */
                const uint32_t third = p.size() >= 3 ? (uint32_t)(uint8_t)p[2] : t;
                const uint32_t w24 = w16 | (third << 16);
                std::vector<uint32_t> &l = lists[KMP_MULTI_HASH(w24 & bmask)];
                if (l.empty() || l.back() != u) l.push_back(u);
                if (p.size() >= 3) break;
            }
            if (p.size() <= KMP_MULTI_SHORT_LEN) continue;
            const uint32_t cl = cls_of[u];
            if (h.classed) {
                uint32_t *rec = tab.data() + KMP_MULTI_REC_W0 + KMP_MULTI_CLS_WORDS + (size_t)(rec_base[cl] + in_cls[u] - cls_short[cl]) * KMP_MULTI_CREC_WORDS;
                rec[0] = (uint32_t)(uint8_t)p[3] | ((uint32_t)p.size() << 8) | (first_pat[h.gidx[u]] << 16);      /* byte 3 (the entry has bytes 0-2), the length, a pattern that has the rest */
                for (uint32_t b = 4; b < p.size() && b < 8u; b++) rec[1] |= (uint32_t)(uint8_t)p[b] << (8 * (b & 3));
            } else {
                uint32_t *rec = tab.data() + KMP_MULTI_REC_W0 + (size_t)(in_cls[u] - cls_short[0]) * KMP_MULTI_REC_WORDS;
                for (uint32_t b = 0; b < p.size() && b < 8u; b++) {
                    rec[b >> 2] |= (uint32_t)(uint8_t)p[b] << (8 * (b & 3));
                    if (b >= 4u) rec[2] |= 0xFFu << (8 * (b & 3));
                }
                rec[3] = (uint32_t)p.size() | (first_pat[h.gidx[u]] << 8);         /* the rest of it: kmp_pattern_dev[that index].pat */
            }
        }
        uint32_t pos = 0;
        for (uint32_t hh = 0; hh < KMP_MULTI_BUCKETS; hh++) {
            for (size_t q = 0; q < lists[hh].size(); q++) {
                const uint32_t u = lists[hh][q];
                const std::string &p = h.uniq[u];
                const uint32_t third = p.size() >= 3 ? (uint32_t)(uint8_t)p[2] : 0u;      /* never 0x00 inside a pattern */
                const uint32_t ent = (uint32_t)(uint8_t)p[0] | ((uint32_t)(uint8_t)p[1] << 8) | (third << 16) | (in_cls[u] << 24);
                if (q == 0) { bucket[2 * hh] = ent; continue; }       /* the first entry sits in the bucket itself */
                if (pos >= KMP_MULTI_MAX_ENTRIES) return false;
                entry[pos++] = ent;
            }
            const uint32_t extra = lists[hh].empty() ? 0u : (uint32_t)lists[hh].size() - 1u;
            bucket[2 * hh + 1] = (pos - extra) | ((uint32_t)lists[hh].size() << 16);
        }
        /* the patterns this group counts, and the row of each */
        for (const auto &e : elig) {
            const auto &pl = place[e.second];
            if (&hg[pl.first] != &h) continue;
            h.ids.push_back(e.first);
            h.rows.push_back(h.row[pl.second]);
        }
        /* the 1-byte patterns that ride along: rows behind the group's own */
        if (n_ones)
            for (const auto &oi : one_ids) { h.ids.push_back(oi.first); h.rows.push_back(rows_n + oi.second); }
        /* row -> the pattern indices that share it, for the offset records (duplicates are reported one by one) and for the
         * rest of a pattern of nine bytes or more (kmp_pattern_dev[first of them].pat) */
        std::vector<uint32_t> uid_first(rows_n + n_ones + 1, 0u), uid_ids(h.ids.size());
        for (uint32_t r : h.rows) uid_first[r + 1]++;
        for (uint32_t u = 0; u < rows_n + n_ones; u++) uid_first[u + 1] += uid_first[u];
        { std::vector<uint32_t> fill(uid_first.begin(), uid_first.end() - 1);
          for (size_t i = 0; i < h.ids.size(); i++) uid_ids[fill[h.rows[i]]++] = h.ids[i]; }
        s.groups.emplace_back();
        kmp_group_tables &g = s.groups.back();
        g.tables = std::move(tab); g.ids = std::move(h.ids); g.rows = std::move(h.rows);
        g.uid_first = std::move(uid_first); g.uid_ids = std::move(uid_ids);
        g.n_unique = rows_n + n_ones; g.cshift = h.classed ? KMP_MULTI_CLS_SHIFT : cls_short[0]; g.classed = h.classed;
        g.bmask = bmask; g.n_ones = n_ones; g.ones = ones;
        s.n_multi_unique += U;
    }
    s.rest = rest_l;
    s.rest.insert(s.rest.end(), rest_s.begin(), rest_s.end());
    s.rest_long = (uint32_t)rest_l.size(); s.rest_short = (uint32_t)rest_s.size();
    return true;
}
