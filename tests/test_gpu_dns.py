"""kmpgpu_dns_locate / kmpgpu_load_dns (GpuMatcher.dns_locate, .dns_spans, .load_dns) on a real MI355X: the first question of the DNS
message in every payload located on the device, and its dotted name as a packed arena that a second context owns, compared with
tests/dns_model.py exactly -- span records, arena bytes including the zero padding, offsets, lengths, the present bitmap with the bits
at n and above 0, the stats, the index and the launches.

Where the kernels of csrc/kmp_dns.hip take another path:
  L in {0, 11, 16, 17, 18}; i_end in {15, 16, 17, 31, 32}; a length byte as the last byte of a unit, with and without the prefix;
  a 63-byte label; 127 one-byte labels; 255 and 256 wire bytes; c in {64, 0xC0, 0xFF} at the first and at a later label; a label one
  byte past L; QTYPE cut by L; QDCOUNT 0                                                                            cases()
  arenas of 1, 63, 64, 65 and 130 payloads and all cases at once, owned and borrowed with padding and a next slot that continue the
  name, without and with the 2-byte prefix, each located under both flags                                           test_cases
  only_present, no payload present, an empty source                                                                 test_arena_outcomes
Past the grid caps: tests/test_gpu_dns_scale.py.  The command lines: tests/test_dns_cli.py.

No test provokes a fault: every negative case is one the library refuses on the host before it launches anything.

Run on a real MI355X:  python -m pytest tests/test_gpu_dns.py -m gpu
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

from conftest import DATA

pytestmark = pytest.mark.gpu

from gpu_support import attach_slots, reset  # noqa: E402  (torch first)

import decode_model as DM  # noqa: E402
import dns_model as DNS  # noqa: E402
import flow_model as FM  # noqa: E402
import match_model as MM  # noqa: E402
import multithreading_string_matching_amd as K  # noqa: E402
from multithreading_string_matching_amd import _lib  # noqa: E402
from multithreading_string_matching_amd.matcher import (  # noqa: E402
    DNS_FIELD_NAMES, DNS_NONE, DNS_ONLY_PRESENT, DNS_QNAME, DNS_QUERY, DNS_RESPONSE, DNS_SPAN_DTYPE, DNS_TCP_PREFIX, OPT_NONTEMPORAL,
    OPT_WHOLE_PAYLOAD, GpuMatcher, device_count)

EINVAL, ESTATE = -2, -3
ONES = 0xFFFFFFFFFFFFFFFF
LAUNCHES = 5                      # kmpgpu.h: name lengths, two scan kernels, index, gather
LAUNCHES_EMPTY = 3                # ... and where dst ends up without a payload; one more where the locate ran
EMPTY = (np.zeros(0, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint32))
GOLDEN = os.path.join(os.path.dirname(DATA), "dns_qnames.json")
CONT = b"\x01z\x02yx\x00\x00\x01\x00\x01\x00\x00"          # what continues a cut name, and ends it with a question's tail


@pytest.fixture(scope="module")
def src():
    m = GpuMatcher(0)
    yield m
    m.close()


@pytest.fixture(scope="module")
def dst():
    m = GpuMatcher(0)
    yield m
    m.close()


@pytest.fixture(scope="module")
def third():
    m = GpuMatcher(0)
    yield m
    m.close()


def first_diff(a, b):
    d = np.flatnonzero(np.asarray(a) != np.asarray(b))
    return None if len(d) == 0 else (int(d[0]), len(d))


def check_arena(m, want):
    """the context's arena against the model's image: index, payload bytes AND zero padding"""
    n = len(want["len"])
    assert m.arena_info() == (n, int(want["len"].sum(dtype=np.uint64)))
    a, off, ln = m.arena_download()
    if n == 0:
        assert len(off) == len(ln) == 0
        return
    assert len(ln) == n and first_diff(ln, want["len"]) is None, first_diff(ln, want["len"])
    assert first_diff(off, want["off"]) is None
    assert len(a) == len(want["arena"]) + 64
    d = first_diff(a[:len(want["arena"])], want["arena"])
    if d is not None:
        k = int(np.searchsorted(want["off"], d[0], side="right")) - 1
        raise AssertionError(f"{d[1]} bytes differ, the first at {d[0]} = payload {k} + {d[0] - int(want['off'][k])} (length {int(ln[k])})")
    assert not a[len(want["arena"]):].any()


def check_spans(m, payloads, tcp=False, fresh=True):
    """dns_locate and the records it keeps against the model; fresh: the spans are stale or of the other flag, so the kernel runs"""
    stats = m.dns_locate(tcp_prefix=tcp)
    assert m.last_timing().launches == (1 if fresh and payloads else 0)
    assert stats == DNS.locate_stats(payloads, tcp)
    got, want = m.dns_spans(), DNS.spans(payloads, tcp)
    assert got.dtype == DNS_SPAN_DTYPE == DNS.SPAN_DTYPE
    if got.tobytes() != want.tobytes():
        k = next(i for i in range(len(payloads)) if got[i].tobytes() != want[i].tobytes())
        raise AssertionError(f"payload {k} ({payloads[k][:60]!r}, length {len(payloads[k])}, tcp {tcp}): {got[k]}, not {want[k]}")


def names_and_check(dst, src, payloads, only_present=False, tcp=False, located=False):
    """located: this call has to make the spans first"""
    want = DNS.load_dns(payloads, only_present, tcp)
    res = dst.load_dns(src, only_present=only_present, tcp_prefix=tcp)
    assert first_diff(res["present"], want["present"]) is None, first_diff(res["present"], want["present"])
    assert np.array_equal(res["index"], want["index"]) and res["index"].dtype == np.int64
    assert res["stats"] == want["stats"]
    check_arena(dst, want)
    t = dst.last_timing()
    assert t.launches == (LAUNCHES if want["payloads"] else LAUNCHES_EMPTY) + (1 if located else 0) and t.kernel_ms > 0
    return want


def everything(dst, src, payloads):
    """both flags: the locate (which runs for each, the spans being of the other flag), once more without a launch, and both modes"""
    for tcp in (False, True):
        check_spans(src, payloads, tcp)
        check_spans(src, payloads, tcp, fresh=False)
        names_and_check(dst, src, payloads, False, tcp)
        names_and_check(dst, src, payloads, True, tcp)


# ------------------------------------------------------------------------------------------------
# 1. the cases of the definition
# ------------------------------------------------------------------------------------------------
def lab(n, salt=0):
    return bytes(0x61 + (i + salt) % 26 for i in range(n))


def cases():
    """(full, L): the payload is full[:L]; what lies behind L in `full` continues the message, and is what a borrowed arena keeps in the
    padding and the next slot"""
    out = []
    root = DNS.message([])
    out += [(root + CONT, L) for L in (0, 11, 16, 17, 18)]                                      # L; 17 is the root question
    for i_end in (15, 16, 17, 31, 32):                                                           # names that end at a unit's edge
        one = DNS.message([lab(i_end - 13, i_end)], tail=b"tail")
        two = DNS.message([lab(1), lab(i_end - 15, i_end)] if i_end >= 16 else [lab(i_end - 13)], flags=0x8180, an=1)
        assert DNS.locate(one)["i_end"] == DNS.locate(two)["i_end"] == i_end
        out += [(one, len(one)), (one, len(one) - 4), (two, len(two))]
    for at in (15, 29, 31, 45, 47, 63):                              # a length byte as a unit's last byte: 15 / 31 / 47 / 63, less the prefix's 2
        m = DNS.message([lab(at - 13, at), lab(5, at), lab(17 if at % 4 == 3 else 2, 3)], qtype=28)
        assert m[at] == 5
        out.append((m, len(m)))
    out.append((DNS.message([lab(63), lab(63, 1), lab(1)], qtype=255), None))                    # 63-byte labels
    out.append((DNS.message([b"x"] * 127), None))                                                # 127 one-byte labels: 255 bytes on the wire
    out.append((DNS.message([lab(61), lab(63, 2), lab(63, 3), lab(63, 4)]), None))               # 255 bytes on the wire
    out.append((DNS.message([lab(62), lab(63, 2), lab(63, 3), lab(63, 4)]), None))               # 256: NONE
    out.append((DNS.message([b"y"] * 126 + [b"yz"]), None))                                      # 256: NONE
    assert [DNS.locate(f) is not None for f, _ in out[-4:]] == [True, True, False, False]
    assert [len(f) - 16 for f, _ in out[-4:]] == [255, 255, 256, 256]
    for c in (64, 0xC0, 0xFF):                                                                   # pointers and reserved label types
        body = bytes([c]) + b"\x0c" + lab(70) + b"\x00\x00\x01\x00\x01" + bytes(200)
        out.append((DNS.message([])[:12] + body, None))
        out.append((DNS.message([])[:12] + b"\x03www" + body, None))
        out.append((DNS.message([])[:12] + b"\x10" + lab(16) + body, None))                       # ... found in the second unit
    for name in ([lab(5)], [lab(3), lab(12)], [lab(20), lab(9), lab(2)]):
        m = DNS.message(name) + CONT
        q_end = DNS.locate(m)["q_end"]
        out += [(m, q_end - 1), (m, q_end - 4), (m, q_end - 5), (m, q_end - 6), (m, q_end)]       # QTYPE cut; the closing byte cut; a label one byte past L
    out.append((DNS.message([lab(7)], qd=0), None))                                              # QDCOUNT 0
    out.append((DNS.message([lab(7)], qd=2, tail=b"\x03two\x00\x00\x01\x00\x01"), None))          # QDCOUNT 2: the first question
    out.append((DNS.message([b"a.b", b"\x00C", b"UPPER%20"], flags=0xFFFF, ident=0xFFFF, qtype=0xFFFF, qclass=0xFFFE, an=0xABCD, ns=0x1234, ar=0xFEDC), None))
    out += [(b"GET / HTTP/1.1\r\n\r\n" + lab(40), None), (bytes(64), None), (b"\xff" * 48, None)]
    return [(f, len(f) if L is None else L) for f, L in out]


def arena_of(cs, tcp, borrowed):
    """payloads and, for a borrowed arena, slots whose padding and next slot continue every cut message"""
    payloads, slots = [], []
    for full, L in cs:
        if tcp:
            full, L = b"\x12\x34" + full, (L + 2 if L else 0)
        full = full + CONT * 3
        p = full[:L]
        payloads.append(p)
        slots.append(full[:max(16, (L + 15) & ~15)])
        if borrowed and L and L % 16 == 0:                                                       # the next slot begins with what would continue it
            nxt = full[L:L + 20]
            payloads.append(nxt)
            slots.append((nxt + CONT * 3)[:32])
    return payloads, (slots if borrowed else None)


@pytest.mark.parametrize("borrowed", [False, True])
@pytest.mark.parametrize("tcp", [False, True])
def test_cases(src, dst, tcp, borrowed):
    cs = cases()
    payloads, slots = arena_of(cs, tcp, borrowed)
    if borrowed:
        # a read behind L changes the verdict: with the slot's bytes in the payload's place the model decides otherwise
        flipped = sum((DNS.locate(t, tcp) is None) != (DNS.locate(s, tcp) is None) for t, s in zip(payloads, slots))
        joined = sum(DNS.locate(t, tcp) is None and DNS.locate(t + payloads[k + 1], tcp) is not None
                     for k, t in enumerate(payloads[:-1]) if len(t) and len(t) % 16 == 0)
        assert flipped >= 8 and joined >= 1, (flipped, joined)
    kinds = DNS.spans(payloads, tcp)["kind"]
    assert {int(k) for k in kinds} == {DNS.NONE, DNS.QUERY, DNS.RESPONSE}
    try:
        reset(src, dst)
        groups = [payloads] + [[payloads[(7 * n + i) % len(payloads)] for i in range(n)] for n in (1, 63, 64, 65, 130)]
        for g in groups:
            sl = None
            if borrowed:
                by = dict(zip(payloads, slots))
                sl = [by[t] for t in g]
            keep = attach_slots(src, g, sl) if borrowed else src.load_arena(K.HostArena.from_payloads(g))
            everything(dst, src, g)
            del keep
    finally:
        reset(src, dst)
        src.load_arena(*EMPTY)


@pytest.mark.parametrize("nontemporal", [1, 0])
def test_random_messages(src, dst, nontemporal):
    """names of 0 .. 12 labels of arbitrary bytes, every start and length of the gather's units, cut messages and noise"""
    rng = np.random.default_rng(91)
    payloads = []
    for k in range(700):
        labels = [rng.integers(0, 256, int(rng.integers(1, 64 if k % 7 == 0 else 14)), dtype=np.uint8).tobytes() for _ in range(int(rng.integers(0, 13)))]
        p = DNS.message(labels, qtype=int(rng.integers(0, 65536)), flags=int(rng.integers(0, 65536)), qd=int(rng.integers(0, 3)),
                        tail=rng.integers(0, 256, int(rng.integers(0, 60)), dtype=np.uint8).tobytes(), tcp_prefix=bool(k % 2))
        payloads.append(p[:int(rng.integers(0, len(p) + 1))] if k % 5 == 0 else p)
    lens = {DNS.locate(p, t)["name_len"] for p in payloads for t in (False, True) if DNS.locate(p, t)}
    assert {0, 1, 15, 16, 17, 31, 32, 33} <= lens and max(lens) > 200
    try:
        reset(src, dst)
        dst.set_option(OPT_NONTEMPORAL, nontemporal)
        src.load_arena(K.HostArena.from_payloads(payloads))
        everything(dst, src, payloads)
    finally:
        reset(src, dst)


def test_arena_outcomes(src, dst):
    g = _lib.gpu_lib()
    msgs = [DNS.message([lab(4), lab(3)]), b"no dns", DNS.message([]), b"", DNS.message([lab(30)], flags=0x8000)]
    try:
        reset(src, dst)
        src.load_arena(K.HostArena.from_payloads(msgs))
        want = names_and_check(dst, src, msgs, only_present=True, located=True)
        assert want["payloads"] == [lab(4) + b"." + lab(3), b"", lab(30)] and want["index"].tolist() == [0, 2, 4]
        # no payload present: dst without an arena, three launches and the locate
        none = [b"dns", b"", bytes(40), DNS.message([lab(3)], qd=0)]
        src.load_arena(K.HostArena.from_payloads(none))
        names_and_check(dst, src, none, only_present=True, located=True)
        assert dst.arena_info() == (0, 0)
        names_and_check(dst, src, none, only_present=False)
        assert dst.arena_info() == (4, 0)
        # an empty source
        src.load_arena(*EMPTY)
        st = _lib.FieldsStats()
        d_present = C.c_void_p(1)
        assert g.kmpgpu_load_dns(dst._ctx, src._ctx, DNS_QNAME, DNS_ONLY_PRESENT, None, C.byref(d_present), C.byref(st)) == 0
        assert dst.arena_info() == (0, 0) and st.n_payloads == 0 and not d_present.value
        res = dst.load_dns(src)
        assert res["present"].shape == (0,) and res["index"].shape == (0,) and res["stats"]["n_payloads"] == 0
        assert src.dns_locate() == {"n_queries": 0, "n_responses": 0, "n_root": 0, "name_bytes": 0} and src.dns_spans().shape == (0,)
    finally:
        reset(src, dst)


# ------------------------------------------------------------------------------------------------
# 2. the fixtures
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def very_big():
    host = K.HostArena.from_pcap(os.path.join(DATA, "very_big_udp.pcap"), "udp", with_meta=True)
    return host, [bytes(host.payload(k)) for k in range(host.n_pkts)]


def name_table(m):
    a, off, ln = m.arena_download()
    names = {}
    for o, l in zip(off.tolist(), ln.tolist()):
        key = a[o:o + l].tobytes().decode("latin-1")
        names[key] = names.get(key, 0) + 1
    return names


@pytest.mark.parametrize("pcap", ["very_big_udp.pcap", "big_udp.pcap"])
def test_fixtures_against_the_model_and_the_golden_table(src, dst, pcap):
    with open(GOLDEN) as f:
        gold = json.load(f)["fixtures"][pcap]
    host = K.HostArena.from_pcap(os.path.join(DATA, pcap), "udp")
    payloads = [bytes(host.payload(k)) for k in range(host.n_pkts)]
    try:
        reset(src, dst)
        src.load_arena(host)
        check_spans(src, payloads)
        st = src.dns_locate()
        assert (st["n_queries"], st["n_responses"], st["name_bytes"]) == (gold["queries"], gold["responses"], gold["name_bytes"])
        names_and_check(dst, src, payloads, only_present=True)
        assert dst.arena_info()[0] == gold["accepted"] and name_table(dst) == gold["names"]
        names_and_check(dst, src, payloads)
    finally:
        reset(src, dst)


def test_youtube_is_in_the_name_buffer_only(src, dst, very_big):
    """the case the buffer is for: `youtube.com` is nowhere in the payloads of very_big_udp.pcap, and in the question of 4 324"""
    host, payloads = very_big
    try:
        reset(src, dst)
        for m in (src, dst):
            m.set_patterns([b"youtube.com"])
        src.load_arena(host)
        for whole in (0, 1):
            src.set_option(OPT_WHOLE_PAYLOAD, whole)
            assert src.scan()[0].tolist() == [0]
        res = dst.load_dns(src)
        assert res["stats"]["n_present"] == len(payloads) == 13768 and res["stats"]["bytes_out"] == 358717
        assert dst.scan()[0].tolist() == [4324]
        assert dst.scan_packets()["pkt_counts"].tolist() == [4324]
    finally:
        reset(src, dst)
        for m in (src, dst):
            m.set_patterns([b"x"])


def test_rule_with_a_header_predicate_and_flows_in_dst(src, dst, very_big):
    """`doubleclick.net` in a question sent to port 53, over the metadata dst carries along; dst's flows are the source's"""
    host, payloads = very_big
    names = [DNS.qname(p) or b"" for p in payloads]
    try:
        reset(src, dst)
        dst.set_patterns([b"doubleclick.net"])
        dst.set_headers([{"dport_lo": 53, "dport_hi": 53, "proto": 17}])
        dst.set_rules([([0, dst.hdr(0)], [])])
        src.load_arena(host)
        assert src.meta().tobytes() == host.meta.tobytes()
        src.build_flows()
        ids = src.flow_ids()
        dst.load_dns(src)
        assert dst.meta().tobytes() == host.meta.tobytes()
        want = np.array([b"doubleclick.net" in t for t in names]) & (host.meta["dst_port"] == 53) & (host.meta["proto"] == 17)
        assert 0 < want.sum() < sum(b"doubleclick.net" in t for t in names)                      # the answers come FROM port 53
        res = dst.scan_rules(hits=True)
        assert np.array_equal(res["hits"][0], want) and res["rule_pkt_counts"].tolist() == [int(want.sum())]
        dst.build_flows()
        assert np.array_equal(dst.flow_ids(), ids) and np.array_equal(ids, FM.flow_of_np(host.meta))
        # only the present ones: their records, in their new order
        pick = np.arange(len(payloads)) % 3 == 0
        third_payloads = [p if k else b"junk" for p, k in zip(payloads[:600], pick)]
        src.load_arena(K.HostArena.from_payloads(third_payloads))
        src.set_meta(host.meta[:600])
        res = dst.load_dns(src, only_present=True)
        assert np.array_equal(res["index"], np.flatnonzero(pick[:600])) and dst.meta().tobytes() == host.meta[:600][pick[:600]].tobytes()
    finally:
        reset(src, dst)
        dst.set_headers(None)
        dst.set_patterns([b"x"])


# ------------------------------------------------------------------------------------------------
# 3. the cache, the source, the errors
# ------------------------------------------------------------------------------------------------
def mixed(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        if k % 4 == 3:
            out.append(rng.integers(0, 256, int(rng.integers(0, 90)), dtype=np.uint8).tobytes())
        else:
            out.append(DNS.message([lab(int(rng.integers(1, 30)), k + i) for i in range(int(rng.integers(0, 6)))], flags=0x8180 if k % 2 else 0x0100,
                                   tail=lab(int(rng.integers(0, 30))), tcp_prefix=k % 8 == 0))
    return out


def test_spans_life_cycle(src, dst, third):
    """a second locate launches nothing, the other flag one kernel; dropped by every loader (load_selected into the source among them),
    kept by a scan; read in ranges; refused where there are none; the HTTP spans live beside them"""
    g = _lib.gpu_lib()
    a, b = mixed(150, seed=92), mixed(90, seed=93)
    out = np.zeros(4, dtype=DNS_SPAN_DTYPE)
    try:
        reset(src, dst, third)
        src.set_patterns([lab(3)])
        src.load_arena(K.HostArena.from_payloads(a))
        assert g.kmpgpu_dns_spans_read(src._ctx, out.ctypes.data, 0, 1) == ESTATE and b"no spans" in g.kmpgpu_last_error()
        names_and_check(dst, src, a, located=True)
        assert src.dns_spans().tobytes() == DNS.spans(a).tobytes()
        check_spans(src, a, fresh=False)                                          # a second locate launches 0
        check_spans(src, a, tcp=True)                                             # the other prefix flag launches 1
        check_spans(src, a, tcp=True, fresh=False)
        names_and_check(dst, src, a, tcp=False, located=True)                     # ... and so does a load with the first flag again
        assert g.kmpgpu_dns_spans_read(src._ctx, out.ctypes.data, 146, 4) == 0 and out.tobytes() == DNS.spans(a[146:]).tobytes()
        assert g.kmpgpu_dns_spans_read(src._ctx, out.ctypes.data, 147, 4) == EINVAL and g.kmpgpu_dns_spans_read(src._ctx, None, 0, 1) == EINVAL
        assert g.kmpgpu_dns_spans_read(None, out.ctypes.data, 0, 1) == EINVAL and g.kmpgpu_dns_locate(None, 0, None) == EINVAL
        assert g.kmpgpu_dns_locate(src._ctx, 1, None) == EINVAL and g.kmpgpu_dns_locate(src._ctx, 4, None) == EINVAL
        assert b"flag bits" in g.kmpgpu_last_error()
        src.http_locate()                                                         # the HTTP spans do not touch them
        src.scan()
        src.scan_packets()
        names_and_check(dst, src, a, only_present=True)                           # a scan keeps them
        third.load_arena(K.HostArena.from_payloads(b))
        pick = np.arange(len(b)) % 2 == 0
        src.load_selected(third, pick)                                            # load_selected into the source drops them
        assert g.kmpgpu_dns_spans_read(src._ctx, out.ctypes.data, 0, 1) == ESTATE
        kept = [t for t, p in zip(b, pick) if p]
        names_and_check(dst, src, kept, located=True)
        check_spans(src, kept, fresh=False)
        assert g.kmpgpu_dns_spans_read(dst._ctx, out.ctypes.data, 0, 1) == ESTATE              # dst's own are not src's
        src.load_arena(K.HostArena.from_payloads(b))                              # a loader drops them
        assert g.kmpgpu_dns_spans_read(src._ctx, out.ctypes.data, 0, 1) == ESTATE
        # a name buffer is a source like any other
        names_and_check(dst, src, b, located=True)
        names_and_check(third, dst, DNS.load_dns(b)["payloads"], located=True)
        # the pairs of the profile: the locate, then lengths, scan, index, gather
        src.load_arena(K.HostArena.from_payloads(a))
        dst.profile_begin(8)
        dst.load_dns(src)
        ms = dst.profile_end(8)
        assert len(ms) == 5 and (ms >= 0).all()
        src.profile_begin(4)
        src.dns_locate(tcp_prefix=True)
        assert len(src.profile_end(4)) == 1
    finally:
        reset(src, dst, third)
        src.set_patterns([b"x"])


def test_src_untouched(src, dst):
    payloads = mixed(300, seed=94)
    pats = [lab(3), b"\x81\x80", lab(2, 1)]
    try:
        reset(src, dst)
        src.set_patterns(pats)
        src.set_option(OPT_WHOLE_PAYLOAD, 1)
        src.load_arena(K.HostArena.from_payloads(payloads))
        before, arena_before = src.scan_packets(hits=True), src.arena_download()
        assert before["counts"].tolist() == list(MM.counts(MM.starts(payloads, pats, whole=True))) and any(before["counts"])
        everything(dst, src, payloads)
        after, arena_after = src.scan_packets(hits=True), src.arena_download()
        assert all(np.array_equal(before[f], after[f]) for f in ("hits", "any", "pkt_counts", "counts"))
        assert all(np.array_equal(x, y) for x, y in zip(arena_before, arena_after))
    finally:
        reset(src, dst)
        src.set_patterns([b"x"])


def test_errors(src, dst):
    g = _lib.gpu_lib()
    payloads = mixed(120, seed=95)
    kept = mixed(77, seed=96)
    want_kept = dict(zip(("arena", "off", "len"), DM.packed_image(kept)))
    st = _lib.FieldsStats()
    d_present = C.c_void_p()
    words = np.zeros(8, dtype=np.uint64)

    def call(d, s, field=DNS_QNAME, flags=0):
        st.n_payloads = 12345
        d_present.value = 1
        return g.kmpgpu_load_dns(d, s, field, flags, words.ctypes.data, C.byref(d_present), C.byref(st))

    def dst_keeps_its_arena(rc, code, what):
        assert rc == code, (rc, code)
        msg = g.kmpgpu_last_error()
        assert b"kmpgpu_load_dns" in msg and what in msg, msg
        assert st.n_payloads == 0 and not d_present.value
        check_arena(dst, want_kept)

    try:
        reset(src, dst)
        src.load_arena(K.HostArena.from_payloads(payloads))
        dst.load_arena(K.HostArena.from_payloads(kept))
        dst_keeps_its_arena(call(dst._ctx, dst._ctx), EINVAL, b"same context")
        dst_keeps_its_arena(call(None, src._ctx), EINVAL, b"ctx is NULL")
        dst_keeps_its_arena(call(dst._ctx, None), EINVAL, b"ctx is NULL")
        dst_keeps_its_arena(call(dst._ctx, src._ctx, field=0), EINVAL, b"field 0")
        dst_keeps_its_arena(call(dst._ctx, src._ctx, field=2), EINVAL, b"field 2")
        dst_keeps_its_arena(call(dst._ctx, src._ctx, flags=4), EINVAL, b"flag bits")
        dst_keeps_its_arena(call(dst._ctx, src._ctx, flags=0x80000001), EINVAL, b"flag bits")
        assert g.kmpgpu_dns_spans_read(src._ctx, words.ctypes.data, 0, 1) == ESTATE          # none of these made the spans
        with pytest.raises(ValueError):
            dst.load_dns(src, field="rdata")
        # between kmpgpu_load_frames_begin and _finish, on either side
        path = os.path.join(DATA, "udp_1000.pcap")
        fr = _lib.Frames()
        err = C.create_string_buffer(_lib.KMP_PCAP_ERRBUF)
        assert _lib.host_lib().kmp_frames_from_pcap(path.encode(), None, None, C.byref(fr), err) == 0
        try:
            with GpuMatcher(0) as other:
                other.set_patterns([b"ab"])
                assert g.kmpgpu_load_frames_begin(other._ctx, fr.bytes, fr.nbytes, fr.off, fr.caplen, fr.n, 0) == 0
                dst_keeps_its_arena(call(dst._ctx, other._ctx), ESTATE, b"src sits between")
                assert call(other._ctx, src._ctx) == ESTATE and b"dst sits between" in g.kmpgpu_last_error()
                assert g.kmpgpu_dns_locate(other._ctx, 0, None) == ESTATE and b"kmpgpu_dns_locate" in g.kmpgpu_last_error()
                n_pay = C.c_uint64()
                assert g.kmpgpu_load_frames_finish(other._ctx, C.byref(n_pay)) == 0
        finally:
            _lib.host_lib().kmp_frames_free(C.byref(fr))
        # NULL outputs, and the device words with the bits at n and above 0
        assert g.kmpgpu_load_dns(dst._ctx, src._ctx, DNS_QNAME, 0, None, None, None) == 0
        check_arena(dst, DNS.load_dns(payloads))
        assert dst.last_timing().launches == LAUNCHES + 1
        words[:] = np.uint64(ONES)
        assert call(dst._ctx, src._ctx, flags=DNS_ONLY_PRESENT | DNS_TCP_PREFIX) == 0 and d_present.value
        have = DNS.load_dns(payloads, True, True)
        assert np.array_equal(words[:2], have["words"]) and st.n_payloads == st.n_present == len(have["index"])
    finally:
        reset(src, dst)


def test_two_devices_are_refused(src):
    if device_count() < 2:
        pytest.skip("one device")
    g = _lib.gpu_lib()
    with GpuMatcher(1) as far:
        src.load_arena(K.HostArena.from_payloads([DNS.message([b"a"]), b"", b"x" * 40]))
        assert g.kmpgpu_load_dns(far._ctx, src._ctx, DNS_QNAME, 0, None, None, None) == EINVAL
        assert b"kmpgpu_load_dns" in g.kmpgpu_last_error() and far.arena_info() == (0, 0)


def test_constants():
    assert DNS_FIELD_NAMES == {"qname": 1} and (DNS_QNAME, DNS_ONLY_PRESENT, DNS_TCP_PREFIX) == (1, 1, 2)
    assert (DNS_NONE, DNS_QUERY, DNS_RESPONSE) == (DNS.NONE, DNS.QUERY, DNS.RESPONSE) == (0, 1, 2)
    assert (K.DNS_QNAME, K.DNS_ONLY_PRESENT, K.DNS_TCP_PREFIX) == (1, 1, 2)
