"""tests/dns_model.py -- the definition of kmpgpu_dns_locate / kmpgpu_load_dns (include/kmpgpu.h) in plain Python -- held to hand-written
verdicts, one per clause of the definition, to dnspython where it is installed, and to the golden table of the two UDP fixtures
(tests/golden/dns_qnames.json, written by tests/golden/make_dns_goldens.py).  No GPU needed."""
import json
import os
import struct

import numpy as np
import pytest

from conftest import DATA

import dns_model as DNS
import multithreading_string_matching_amd as K

GOLDEN = os.path.join(os.path.dirname(DATA), "dns_qnames.json")
HDR = struct.pack(">6H", 0xBEEF, 0x0100, 1, 0, 0, 0)
Q = b"\x00\x01\x00\x01"                 # QTYPE A, QCLASS IN


def fixture_payloads(pcap):
    arena = K.HostArena.from_pcap(os.path.join(DATA, pcap), "udp")
    return [bytes(arena.payload(k)) for k in range(arena.n_pkts)]


def test_hand_written_verdicts():
    www = b"\x03www\x07youtube\x03com\x00"
    t = DNS.locate(HDR + www + Q)
    assert t["name"] == b"www.youtube.com" and (t["kind"], t["n_labels"], t["id"], t["flags"]) == (DNS.QUERY, 3, 0xBEEF, 0x0100)
    assert (t["qtype"], t["qclass"], t["qdcount"], t["name_off"], t["name_len"], t["q_end"], t["i_end"]) == (1, 1, 1, 13, 15, 33, 28)
    # M >= 17: the root question is the smallest message
    root = HDR + b"\x00" + Q
    assert len(root) == 17 and DNS.qname(root) == b"" and DNS.locate(root)["q_end"] == 17 and DNS.locate(root)["n_labels"] == 0
    assert DNS.locate(root[:16]) is None and DNS.locate(b"") is None and DNS.locate(root[:11]) is None
    assert DNS.qname(root + b"x") == b""
    # QDCOUNT >= 1
    assert DNS.locate(HDR[:4] + b"\x00\x00" + HDR[6:] + www + Q) is None
    assert DNS.locate(HDR[:4] + b"\x01\x00" + HDR[6:] + www + Q)["qdcount"] == 256
    # i_t < M: the walk runs out of the payload in front of a length byte
    assert DNS.locate(HDR + b"\x03www\x07youtube") is None
    # c >= 64 at the first and at a later label
    for c in (64, 0xC0, 0xFF):
        assert DNS.locate(HDR + bytes([c]) + b"\x0c" + Q + b"\x00" * 300) is None
        assert DNS.locate(HDR + b"\x03www" + bytes([c]) + b"\x0c" + Q + b"\x00" * 300) is None
    assert DNS.qname(HDR + b"\x3f" + b"a" * 63 + b"\x00" + Q) == b"a" * 63
    # i_t + 1 + c <= M: a label that runs one byte past L, and one that ends at L (then the closing byte is missing)
    assert DNS.locate(HDR + b"\x05abcd") is None and DNS.locate(HDR + b"\x05abcde") is None
    # i_end + 1 - 12 <= 255
    name255 = b"".join(b"\x01x" for _ in range(127)) + b"\x00"
    assert len(name255) == 255 and DNS.qname(HDR + name255 + Q) == b".".join([b"x"] * 127) and DNS.locate(HDR + name255 + Q)["n_labels"] == 127
    name256 = b"\x02xy" + b"".join(b"\x01x" for _ in range(126)) + b"\x00"
    assert len(name256) == 256 and DNS.locate(HDR + name256 + Q) is None
    # i_end + 5 <= M
    assert DNS.locate((HDR + www + Q)[:-1]) is None and DNS.locate(HDR + www + Q) is not None
    # kind: bit 15 of the flags word
    assert DNS.locate(HDR[:2] + b"\x81\x80" + HDR[4:] + www + Q)["kind"] == DNS.RESPONSE
    assert DNS.locate(HDR[:2] + b"\x7f\xff" + HDR[4:] + www + Q)["kind"] == DNS.QUERY
    # bytes as they are: a '.', a 0x00 and upper case inside a label
    assert DNS.qname(HDR + b"\x03a.b\x02\x00C\x00" + Q) == b"a.b.\x00C"
    # the TCP prefix: b = 2, the length in front is not checked
    assert DNS.qname(b"\xff\xff" + HDR + www + Q, tcp_prefix=True) == b"www.youtube.com"
    t = DNS.locate(b"\x00\x00" + HDR + www + Q, tcp_prefix=True)
    assert (t["name_off"], t["q_end"]) == (15, 35) and DNS.locate((b"\x00\x00" + root)[:18], tcp_prefix=True) is None
    assert DNS.span(b"junk") == (0,) * 14 and DNS.spans([root, b""]).tobytes()[32:] == b"\0" * 32


def test_message_builder_and_images():
    p = DNS.message([b"a", b"bc"], qtype=28, ident=7, flags=0x8180, an=2, tail=b"answers")
    t = DNS.locate(p)
    assert (t["name"], t["qtype"], t["id"], t["kind"], t["ancount"]) == (b"a.bc", 28, 7, DNS.RESPONSE, 2)
    assert DNS.locate(DNS.message([b"a"], tcp_prefix=True), tcp_prefix=True)["name"] == b"a"
    payloads = [p, b"not dns", DNS.message([]), DNS.message([b"x" * 20])]
    full, only = DNS.load_dns(payloads), DNS.load_dns(payloads, only_present=True)
    assert full["payloads"] == [b"a.bc", b"", b"", b"x" * 20] and full["present"].tolist() == [True, False, True, True]
    assert only["payloads"] == [b"a.bc", b"", b"x" * 20] and only["index"].tolist() == [0, 2, 3]
    assert full["off"].tolist() == [0, 16, 32, 48] and full["len"].tolist() == [4, 0, 0, 20] and len(full["arena"]) == 80
    assert only["stats"] == {"n_payloads": 3, "n_present": 3, "bytes_in": len(p) + 17 + len(payloads[3]), "bytes_out": 24}
    assert DNS.locate_stats(payloads) == {"n_queries": 2, "n_responses": 1, "n_root": 1, "name_bytes": 24}


def generated(n, seed):
    """messages whose walk meets no byte of 64 or above: 0 .. 12 labels of 1 .. 63 arbitrary bytes, cut anywhere now and then"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        labels = [rng.integers(0, 256, int(rng.integers(1, 64 if k % 7 == 0 else 12)), dtype=np.uint8).tobytes() for _ in range(int(rng.integers(0, 13)))]
        p = DNS.message(labels, qtype=int(rng.integers(0, 65536)), flags=int(rng.integers(0, 65536)), qd=int(rng.integers(0, 3)),
                        tail=rng.integers(0, 256, int(rng.integers(0, 40)), dtype=np.uint8).tobytes())
        out.append(p[:int(rng.integers(0, len(p) + 1))] if k % 5 == 0 else p)
    return out


def test_against_dnspython():
    pytest.importorskip("dns.name")
    import dns.name
    seen = 0
    for payloads in (fixture_payloads("very_big_udp.pcap"), fixture_payloads("big_udp.pcap"), generated(3000, seed=5)):
        for p in payloads:
            t = DNS.locate(p)
            if t is None:
                continue
            name, used = dns.name.from_wire(p, 12)
            assert b".".join(name.labels[:-1]) == t["name"] and used == t["i_end"] + 1 - 12 and len(name.labels) - 1 == t["n_labels"]
            seen += 1
    assert seen > 13768 + 1943 + 1500


@pytest.mark.parametrize("pcap", ["very_big_udp.pcap", "big_udp.pcap"])
def test_golden_table(pcap):
    with open(GOLDEN) as f:
        want = json.load(f)["fixtures"][pcap]
    payloads = fixture_payloads(pcap)
    ts = [t for t in (DNS.locate(p) for p in payloads) if t is not None]
    names = {}
    for t in ts:
        key = t["name"].decode("latin-1")
        names[key] = names.get(key, 0) + 1
    st = DNS.locate_stats(payloads)
    assert (len(payloads), len(ts), st["n_queries"], st["n_responses"], st["name_bytes"]) == \
        (want["payloads"], want["accepted"], want["queries"], want["responses"], want["name_bytes"])
    assert names == want["names"]
    if pcap == "very_big_udp.pcap":
        assert (want["accepted"], want["responses"], want["name_bytes"], len(names)) == (13768, 6855, 358717, 101)
        assert sum(c for s, c in names.items() if "youtube.com" in s) == 4324 and not any(b"youtube.com" in p for p in payloads)
        assert max(t["n_labels"] for t in ts) == 34 and max(t["name_len"] for t in ts) == 72
        assert sum(t["qdcount"] == 2 for t in ts) == 25
    else:
        assert (want["accepted"], want["name_bytes"]) == (1943, 45858)
        assert any("%" in s for s in names) and any(s != s.lower() for s in names)
