/* flows_sanitizer_driver.cpp -- csrc/kmp_flow_key.h on the host, under -fsanitize=address,undefined (tests/test_flows_host.py): the key, the
 * mix and kmp_flow_group, the serial twin of the grouping kmpgpu_flows_build does on the device.
 *
 *   flows_driver <in> <out>
 * in:  uint64 n, uint64 slots (0 = auto), uint32 directed, uint32 0, kmpgpu_pkt_meta[n], uint32 len[n]
 * out: uint64 n_flows (UINT64_MAX: the slot count was refused, nothing follows), uint32 flow_of[n], kmpgpu_flow[n_flows]
 * Without arguments: the hand-written checks below only. */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "kmp_flow_key.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

static kmpgpu_pkt_meta M(uint32_t s, uint32_t d, uint16_t sp, uint16_t dp, uint8_t pr)
{
    kmpgpu_pkt_meta m;
    memset(&m, 0, sizeof m);
    m.src_ip = s; m.dst_ip = d; m.src_port = sp; m.dst_port = dp; m.proto = pr;
    return m;
}

static int hand_checks()
{
    static_assert(sizeof(kmpgpu_flow) == 48 && sizeof(kmpgpu_pkt_meta) == 16, "the records of kmpgpu.h");
    const uint32_t A = 0x0A000001u, B = 0x0B000002u;
    /* the two directions: one key by default, two when directed */
    const kmp_flow_key f = kmp_flow_key_of_meta(M(A, B, 1000, 80, 6), false), r = kmp_flow_key_of_meta(M(B, A, 80, 1000, 6), false);
    CHECK(kmp_flow_key_eq(f, r) && kmp_flow_hash(f) == kmp_flow_hash(r));
    CHECK(f.a == ((uint64_t)A << 16 | 1000) && f.b == ((uint64_t)B << 16 | 80) && f.proto == 6);
    CHECK(!kmp_flow_key_eq(kmp_flow_key_of_meta(M(A, B, 1000, 80, 6), true), kmp_flow_key_of_meta(M(B, A, 80, 1000, 6), true)));
    /* the extremes of every field, and the word the kernels load the ports and the protocol from */
    const kmp_flow_key x = kmp_flow_key_of(0xFFFFFFFFu, 0u, 0xFFFF0000u, 0xABCDEFFFu, false);
    CHECK(x.a == 0xFFFFull && x.b == 0xFFFFFFFF0000ull && x.proto == 0xFF);
    /* reserved is not part of the key */
    kmpgpu_pkt_meta m = M(A, B, 1, 2, 17);
    m.reserved[0] = 1; m.reserved[2] = 0xFF;
    CHECK(kmp_flow_key_eq(kmp_flow_key_of_meta(m, false), kmp_flow_key_of_meta(M(A, B, 1, 2, 17), false)));
    /* A:1 -> B:2 and A:2 -> B:1 */
    CHECK(!kmp_flow_key_eq(kmp_flow_key_of_meta(M(A, B, 1, 2, 17), false), kmp_flow_key_of_meta(M(A, B, 2, 1, 17), false)));
    /* auto slots: the smallest power of two >= 2 n */
    CHECK(kmp_flow_auto_slots(0) == 2 && kmp_flow_auto_slots(1) == 2 && kmp_flow_auto_slots(2) == 4 && kmp_flow_auto_slots(3) == 8);
    CHECK(kmp_flow_auto_slots(512) == 1024 && kmp_flow_auto_slots(513) == 2048 && kmp_flow_auto_slots(0xFFFFFFFEull) == (1ull << 32));
    /* a table that is full but for one slot: every probe chain wraps and ends */
    std::vector<kmpgpu_pkt_meta> meta;
    std::vector<uint32_t> len, flow_of;
    std::vector<kmpgpu_flow> recs;
    for (uint32_t i = 0; i < 127; ++i) { meta.push_back(M(A + i, B, 7, 7, 17)); len.push_back(i); }
    for (uint32_t i = 0; i < 127; ++i) { meta.push_back(M(B, A + i, 7, 7, 17)); len.push_back(1000); }       /* the answers */
    CHECK(kmp_flow_group(meta.data(), len.data(), 254, false, 256, &flow_of, &recs) == 127);
    for (uint32_t i = 0; i < 254; ++i) CHECK(flow_of[i] == i % 127);
    for (uint32_t i = 0; i < 127; ++i)
        CHECK(recs[i].first_packet == i && recs[i].last_packet == i + 127 && recs[i].n_packets == 2 && recs[i].payload_bytes == i + 1000 &&
              recs[i].first.src_ip == A + i);
    CHECK(kmp_flow_group(meta.data(), len.data(), 254, true, 256, &flow_of, &recs) == 254);
    /* refused slot counts; no payloads */
    CHECK(kmp_flow_group(meta.data(), len.data(), 254, false, 254, &flow_of, &recs) == UINT64_MAX);
    CHECK(kmp_flow_group(meta.data(), len.data(), 254, false, 128, &flow_of, &recs) == UINT64_MAX);
    CHECK(kmp_flow_group(meta.data(), len.data(), 254, false, 384, &flow_of, &recs) == UINT64_MAX);
    CHECK(kmp_flow_group(nullptr, nullptr, 0, false, 0, &flow_of, &recs) == 0 && flow_of.empty() && recs.empty());
    return 0;
}

int main(int argc, char **argv)
{
    if (hand_checks()) return 1;
    if (argc == 3) {
        FILE *in = fopen(argv[1], "rb");
        CHECK(in);
        uint64_t n = 0, slots = 0;
        uint32_t directed[2] = {0, 0};
        CHECK(fread(&n, 8, 1, in) == 1 && fread(&slots, 8, 1, in) == 1 && fread(directed, 4, 2, in) == 2);
        std::vector<kmpgpu_pkt_meta> meta((size_t)n);
        std::vector<uint32_t> len((size_t)n), flow_of;
        std::vector<kmpgpu_flow> recs;
        CHECK(fread(meta.data(), sizeof(kmpgpu_pkt_meta), (size_t)n, in) == n && fread(len.data(), 4, (size_t)n, in) == n);
        fclose(in);
        const uint64_t nf = kmp_flow_group(meta.data(), len.data(), n, directed[0] != 0, slots, &flow_of, &recs);
        FILE *out = fopen(argv[2], "wb");
        CHECK(out);
        CHECK(fwrite(&nf, 8, 1, out) == 1);
        if (nf != UINT64_MAX) {
            CHECK(fwrite(flow_of.data(), 4, (size_t)n, out) == n && fwrite(recs.data(), sizeof(kmpgpu_flow), (size_t)nf, out) == nf);
        }
        CHECK(fclose(out) == 0);
    } else CHECK(argc == 1);
    printf("flows driver ok\n");
    return 0;
}
