/* kmp_flow_key.h -- the flow key of kmpgpu_flows_build (kmpgpu.h): how a payload's metadata record becomes its key, and the 32-bit mix that
 * picks the key's first slot in the hash table.  Plain C++ that the kernels of kmp_flows.hip and host code both compile, so that the two
 * cannot drift apart; and kmp_flow_group, the same grouping done serially on the host through the same table (the command lines' self-check
 * and tests/flows_sanitizer_driver.cpp call it). */
#ifndef KMP_FLOW_KEY_H
#define KMP_FLOW_KEY_H

#include <stdint.h>

#include <vector>

#include "kmpgpu.h"

#if defined(__HIPCC__)
#define KMP_FK_HD __host__ __device__ __forceinline__
#else
#define KMP_FK_HD inline
#endif

/* key(k) = (proto, a, b): a = e_src, b = e_dst under KMPGPU_FLOW_DIRECTED, otherwise a = min, b = max of the two 48-bit endpoints
 * e = ip << 16 | port.  13 bytes of information; `reserved` is not part of it */
struct kmp_flow_key {
    uint64_t a, b;
    uint32_t proto;
};

/* from the record's four words as the kernels load them: {src_ip, dst_ip, src_port | dst_port << 16, proto | reserved << 8} */
KMP_FK_HD kmp_flow_key kmp_flow_key_of(uint32_t src_ip, uint32_t dst_ip, uint32_t ports, uint32_t w3, bool directed)
{
    const uint64_t es = (uint64_t)src_ip << 16 | (ports & 0xFFFFu), ed = (uint64_t)dst_ip << 16 | (ports >> 16);
    const bool swap = !directed && ed < es;
    kmp_flow_key k;
    k.a = swap ? ed : es;
    k.b = swap ? es : ed;
    k.proto = w3 & 0xFFu;
    return k;
}

KMP_FK_HD bool kmp_flow_key_eq(const kmp_flow_key &x, const kmp_flow_key &y) { return (x.a == y.a) & (x.b == y.b) & (x.proto == y.proto); }

/* the finaliser of MurmurHash3 */
KMP_FK_HD uint32_t kmp_flow_fmix(uint32_t h)
{
    h ^= h >> 16; h *= 0x85EBCA6Bu;
    h ^= h >> 13; h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}

/* the key's 13 bytes as four words (the two 16-bit high parts share one, the protocol byte rides on the last), each finalised into the next */
KMP_FK_HD uint32_t kmp_flow_hash(const kmp_flow_key &k)
{
    uint32_t h = kmp_flow_fmix((uint32_t)k.a ^ 0x9E3779B9u);
    h = kmp_flow_fmix(h ^ (uint32_t)k.b);
    h = kmp_flow_fmix(h ^ ((uint32_t)(k.a >> 32) | (uint32_t)(k.b >> 32) << 16));
    return kmp_flow_fmix(h ^ k.proto);
}

/* KMPGPU_OPT_FLOW_SLOTS = 0: the smallest power of two >= 2 n (2 for n <= 1), at most 2^32: a slot's index is 32 bits wide, and
 * n <= 2^32 - 2 leaves a table of 2^32 slots a free one */
inline uint64_t kmp_flow_auto_slots(uint64_t n)
{
    uint64_t s = 2;
    while (s < 2 * n && s < (1ull << 32)) s <<= 1;
    return s;
}

inline kmp_flow_key kmp_flow_key_of_meta(const kmpgpu_pkt_meta &m, bool directed)
{
    return kmp_flow_key_of(m.src_ip, m.dst_ip, (uint32_t)m.src_port | (uint32_t)m.dst_port << 16, m.proto, directed);
}

/* The grouping of kmpgpu_flows_build, serially: open addressing over `slots` slots (a power of two > n, or 0 for auto) that hold payload
 * index + 1, linear probing from kmp_flow_hash & (slots - 1), wrapping at the end.  flow_of[n], recs[n_flows] as kmpgpu.h defines them;
 * len[k] = L_k.  Returns n_flows, or UINT64_MAX where slots is no power of two above n or n > 2^32 - 2. */
inline uint64_t kmp_flow_group(const kmpgpu_pkt_meta *meta, const uint32_t *len, uint64_t n, bool directed, uint64_t slots,
                               std::vector<uint32_t> *flow_of, std::vector<kmpgpu_flow> *recs)
{
    if (n > 0xFFFFFFFEull) return UINT64_MAX;
    if (slots == 0) slots = kmp_flow_auto_slots(n);
    if ((slots & (slots - 1)) || slots <= n || slots > (1ull << 32)) return UINT64_MAX;
    std::vector<uint32_t> table((size_t)slots, 0u), id_of((size_t)slots, 0u);
    flow_of->assign((size_t)n, 0u);
    recs->clear();
    for (uint64_t k = 0; k < n; ++k) {
        const kmp_flow_key key = kmp_flow_key_of_meta(meta[k], directed);
        uint64_t s = kmp_flow_hash(key) & (slots - 1);
        while (table[s] && !kmp_flow_key_eq(key, kmp_flow_key_of_meta(meta[table[s] - 1u], directed))) s = (s + 1) & (slots - 1);
        if (!table[s]) {
            /* payloads come in order: the one that takes the slot is the flow's first, and flows are numbered as they appear */
            table[s] = (uint32_t)k + 1u;
            id_of[s] = (uint32_t)recs->size();
            kmpgpu_flow f;
            f.first_packet = f.last_packet = k;
            f.n_packets = 0; f.payload_bytes = 0;
            f.first = meta[k];
            recs->push_back(f);
        }
        kmpgpu_flow &f = (*recs)[id_of[s]];
        (*flow_of)[k] = id_of[s];
        f.last_packet = k;
        f.n_packets++;
        f.payload_bytes += len[k];
    }
    return recs->size();
}

#endif
