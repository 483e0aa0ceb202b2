"""tests/tls_model.py -- the definition of kmpgpu_tls_locate / kmpgpu_load_tls (include/kmpgpu.h) in plain Python -- held to hand-written
verdicts, one per "NONE unless" clause of the definition at the value that just passes and the value that just fails, to the ClientHellos
OpenSSL wrote (tests/golden/tls_hellos.json, made by tests/golden/make_tls_goldens.py), and to every prefix of them.  No GPU needed."""
import importlib.util
import json
import os
import struct

import pytest

from conftest import DATA

import tls_model as TLS

GOLDEN_DIR = os.path.dirname(DATA)
GOLDEN = os.path.join(GOLDEN_DIR, "tls_hellos.json")
H, SNI, ALPN, EXT = TLS.hello, TLS.sni_ext, TLS.alpn_ext, TLS.ext


def golden_hellos():
    with open(GOLDEN) as f:
        return json.load(f)["hellos"]


def patched(p: bytes, pos: int, byte: int) -> bytes:
    return p[:pos] + bytes([byte]) + p[pos + 1:]


def test_fixed_header():
    p = H([SNI(b"example.com")])
    t = TLS.locate(p)
    assert t["sni"] == b"example.com" and t["alpn"] is None and t["flags"] == TLS.HAS_SNI and t["n_ext"] == 1
    assert (t["record_version"], t["client_version"], t["sid_len"], t["n_suites"], t["hs_len"]) == (0x0301, 0x0303, 32, 3, len(p) - 9)
    assert t["sni_off"] == p.index(b"example.com") and t["sni_len"] == 11
    # p[0] == 22, p[1] == 3, p[2] <= 4, p[5] == 1, p[9] == 3
    for pos, good, bad in ((0, 22, 21), (0, 22, 23), (1, 3, 2), (1, 3, 4), (2, 4, 5), (2, 0, 5), (5, 1, 0), (5, 1, 2), (9, 3, 2), (9, 3, 4)):
        assert TLS.locate(patched(p, pos, good)) is not None and TLS.locate(patched(p, pos, bad)) is None, (pos, good, bad)
    assert TLS.locate(patched(p, 2, 4))["record_version"] == 0x0304 and TLS.locate(patched(p, 10, 0xFF))["client_version"] == 0x03FF
    # rec >= hs + 4
    hs = len(p) - 9
    assert TLS.locate(H([SNI(b"example.com")], rec=hs + 4)) is not None and TLS.locate(H([SNI(b"example.com")], rec=hs + 3)) is None
    assert TLS.locate(H([SNI(b"example.com")], rec=0xFFFF)) is not None
    # L >= 11, and nothing of a short payload is looked at
    assert TLS.locate(p[:11]) is None and TLS.locate(p[:10]) is None and TLS.locate(b"") is None
    assert TLS.span(b"junk") == (0,) * 13 and TLS.spans([p, b""]).tobytes()[32:] == b"\0" * 32


def test_fixed_part():
    # 43 < E: by L and by H
    p = H([SNI(b"a.b")])
    assert TLS.locate(p[:43]) is None and TLS.locate(p[:44]) is None          # (44: c + 2 <= E fails next)
    assert TLS.locate(H(hs=34)) is None and TLS.locate(H(hs=35)) is None      # H = 43, 44
    # sid <= 32
    assert TLS.locate(H([SNI(b"a.b")], sid=32)) is not None and TLS.locate(H([SNI(b"a.b")], sid=32, sid_byte=33)) is None
    assert TLS.locate(H([SNI(b"a.b")], sid=0))["sid_len"] == 0
    # c + 2 <= E at the cipher suites' length
    q = H([SNI(b"a.b")], sid=0)
    assert TLS.locate(q[:45]) is None and TLS.locate(q[:46]) is None
    # cs even and >= 2
    assert TLS.locate(H(suites=1))["n_suites"] == 1 and TLS.locate(H(suites=0)) is None
    assert TLS.locate(H(suites=2, cs=3)) is None and TLS.locate(H(suites=2, cs=1)) is None
    # c < E at the compression methods' length: a hello cut right in front of it, and right behind it
    cut = 44 + 2 + 2                                                          # sid 0, one suite
    r = H([SNI(b"a.b")], sid=0, suites=1)
    assert TLS.locate(r[:cut]) is None and TLS.locate(r[:cut + 1]) is None    # (cut + 1: c != H and c + 2 > E)
    # cm >= 1
    assert TLS.locate(H(cm=b"")) is None and TLS.locate(H(cm=b"\x00"))["n_ext"] == 0 and TLS.locate(H(cm=b"\x01\x00")) is not None
    # c == H: no extensions, valid, both fields absent, never truncated
    t = TLS.locate(H(no_ext_block=True))
    assert t is not None and t["flags"] == 0 and t["sni"] is None and t["alpn"] is None
    assert TLS.locate(H(no_ext_block=True, tail=b"\x17\x03\x03\x00\x01x"))["flags"] == 0
    # otherwise c + 2 <= E and X == H
    full = H([SNI(b"a.b")])
    n_fixed = len(H(no_ext_block=True))
    assert TLS.locate(full[:n_fixed + 1]) is None and TLS.locate(full[:n_fixed + 2])["flags"] == TLS.TRUNCATED
    xs = len(SNI(b"a.b"))
    assert TLS.locate(H([SNI(b"a.b")], xlen=xs - 1)) is None and TLS.locate(H([SNI(b"a.b")], xlen=xs + 1)) is None
    assert TLS.locate(H([SNI(b"a.b")], hs=len(full) - 9 + 1, rec=0xFFFF)) is None      # X == H - 1
    # an empty extension block is a hello with no extension
    assert TLS.locate(H([]))["n_ext"] == 0 and TLS.locate(H([]))["flags"] == 0


def test_extension_walk():
    # b + n > X makes it NONE; an extension that ends exactly at X counts
    assert TLS.locate(H([EXT(10, b"xy")]))["n_ext"] == 1 and TLS.locate(H([EXT(10, b"xy", n=3)])) is None
    # the walk must end at X: fewer than 4 bytes left over
    assert TLS.locate(H([EXT(10, b"xy"), b"\x00\x00\x00"])) is None and TLS.locate(H([EXT(10, b"xy"), EXT(11, b"")]))["n_ext"] == 2
    # a truncated hello: b + n > Xe ends the walk, whole extensions count
    p = H([EXT(10, b"xy"), SNI(b"example.com"), ALPN([b"h2"])])
    t = TLS.locate(p[:-1])
    assert t["flags"] == TLS.TRUNCATED | TLS.HAS_SNI and t["n_ext"] == 2 and t["sni"] == b"example.com" and t["alpn"] is None
    assert TLS.locate(p)["flags"] == TLS.HAS_SNI | TLS.HAS_ALPN
    # ... and an extension that leaves X makes even a truncated hello NONE
    assert TLS.locate(H([EXT(10, b"xy"), EXT(11, b"abcdef", n=7)])[:-3]) is None
    # 255 extensions count, a 256th makes it NONE
    assert TLS.locate(H([EXT(100 + i, b"") for i in range(255)]))["n_ext"] == 255
    assert TLS.locate(H([EXT(100 + i, b"") for i in range(256)])) is None
    # the first of each wins; a later one is not even looked at
    t = TLS.locate(H([SNI(b"first.example"), SNI(b"second.example"), ALPN([b"h2"]), ALPN([b"h3"]), EXT(0, b"\xff"), EXT(16, b"")]))
    assert t["sni"] == b"first.example" and t["alpn"] == b"h2" and t["n_ext"] == 6
    # both orders, and behind 40 others
    assert TLS.locate(H([ALPN([b"h2"]), SNI(b"a.b")]))["sni"] == b"a.b"
    many = [EXT(100 + i, bytes(i % 7)) for i in range(40)]
    t = TLS.locate(H(many + [ALPN([b"h2", b"http/1.1"]), SNI(b"a.b")]))
    assert (t["sni"], t["alpn"], t["n_ext"], t["n_alpn"]) == (b"a.b", b"h2,http/1.1", 42, 2)


def test_server_name():
    ok = SNI(b"example.com")
    assert TLS.locate(H([ok]))["sni"] == b"example.com"
    # n >= 5
    assert TLS.locate(H([EXT(0, b"\x00\x03\x00\x00\x00")]))["sni"] == b"" and TLS.locate(H([EXT(0, b"\x00\x02\x00\x00")])) is None
    assert TLS.locate(H([EXT(0, b"")])) is None
    # ll + 2 <= n
    assert TLS.locate(H([SNI(b"example.com", ll=14)])) is not None and TLS.locate(H([SNI(b"example.com", ll=15)])) is None
    # p[b + 2] == 0
    assert TLS.locate(H([SNI(b"example.com", name_type=1)])) is None
    # 3 + nl <= ll
    assert TLS.locate(H([SNI(b"example.com", nl=11)]))["sni_len"] == 11 and TLS.locate(H([SNI(b"example.com", nl=12)])) is None
    # the first entry only; a shorter nl takes fewer bytes; nl == 0 is present and empty
    t = TLS.locate(H([SNI(b"example.com", tail=b"\x00\x00\x03b.c")]))
    assert t["sni"] == b"example.com"
    assert TLS.locate(H([SNI(b"example.com", nl=7)]))["sni"] == b"example"
    t = TLS.locate(H([SNI(b"")]))
    assert t["sni"] == b"" and t["flags"] == TLS.HAS_SNI and t["sni_len"] == 0 and t["sni_off"] > 0
    # bytes as they are
    assert TLS.locate(H([SNI(b"ExAmPlE.\x00\xff")]))["sni"] == b"ExAmPlE.\x00\xff"


def test_alpn():
    t = TLS.locate(H([ALPN([b"h2", b"http/1.1"])]))
    assert (t["alpn"], t["n_alpn"], t["alpn_len"], t["flags"]) == (b"h2,http/1.1", 2, 11, TLS.HAS_ALPN)
    assert TLS.locate(H([ALPN([b"h2"])]))["alpn"] == b"h2" and TLS.locate(H([ALPN([b"h2"])]))["n_alpn"] == 1
    # n >= 4, ll + 2 == n, ll >= 2
    assert TLS.locate(H([EXT(16, b"\x00\x02\x01x")]))["alpn"] == b"x"
    assert TLS.locate(H([EXT(16, b"\x00\x01\x00")])) is None and TLS.locate(H([EXT(16, b"\x00\x01\x01x")])) is None
    assert TLS.locate(H([ALPN([b"h2"], ll=2)])) is None and TLS.locate(H([ALPN([b"h2"], ll=4)])) is None
    assert TLS.locate(H([EXT(16, b"\x00\x03\x02h2\x00")])) is None
    # every name 1 .. 255, ending exactly at b + 2 + ll
    assert TLS.locate(H([ALPN([b"h2", 0])])) is None and TLS.locate(H([ALPN([0, b"h2"])])) is None
    assert TLS.locate(H([EXT(16, b"\x00\x05\x02h2\x02x")])) is None and TLS.locate(H([EXT(16, b"\x00\x05\x02h2\x01x")]))["alpn"] == b"h2,x"
    assert TLS.locate(H([ALPN([b"z" * 255])]))["alpn"] == b"z" * 255
    # ll == 256 is the widest list the mask holds; 257 is skipped: absent, and the hello stays one
    t = TLS.locate(H([ALPN([b"a" * 127, b"b" * 127])]))
    assert t["alpn_len"] == 255 and t["alpn"] == b"a" * 127 + b"," + b"b" * 127
    t = TLS.locate(H([ALPN([b"a" * 127, b"b" * 128]), SNI(b"a.b")]))
    assert t["flags"] == TLS.ALPN_SKIPPED | TLS.HAS_SNI and t["alpn"] is None and (t["alpn_off"], t["alpn_len"], t["n_alpn"]) == (0, 0, 0)
    # ... whatever it holds
    assert TLS.locate(H([ALPN([0] * 300)]))["flags"] == TLS.ALPN_SKIPPED
    t = TLS.locate(H([ALPN([b"x"] * 128)]))
    assert t["n_alpn"] == 128 and t["alpn"] == b",".join([b"x"] * 128)


def test_images_and_stats():
    a, b = H([SNI(b"example.com"), ALPN([b"h2", b"http/1.1"])]), H([ALPN([b"h2"])])
    payloads = [a, b"GET / HTTP/1.1\r\n\r\n", b, H([SNI(b"")]), a[:-2], b""]
    full, only = TLS.load_tls(payloads, "sni"), TLS.load_tls(payloads, "sni", only_present=True)
    assert full["payloads"] == [b"example.com", b"", b"", b"", b"example.com", b""]
    assert full["present"].tolist() == [True, False, False, True, True, False] and only["index"].tolist() == [0, 3, 4]
    assert only["payloads"] == [b"example.com", b"", b"example.com"]
    assert only["stats"] == {"n_payloads": 3, "n_present": 3, "bytes_in": 2 * len(a) - 2 + len(payloads[3]), "bytes_out": 22}
    assert TLS.load_tls(payloads, "alpn")["payloads"] == [b"h2,http/1.1", b"", b"h2", b"", b"", b""]
    assert TLS.locate_stats(payloads) == {"n_hellos": 4, "n_sni": 3, "n_alpn": 2, "n_truncated": 1}


def check_hello_and_prefixes(p, sni, alpn):
    t = TLS.locate(p)
    assert t is not None and t["flags"] & TLS.TRUNCATED == 0
    assert t["sni"] == (sni.encode() if sni else None) and t["alpn"] == (",".join(alpn).encode() if alpn else None)
    assert t["hs_len"] + 9 == len(p) == be16(p, 3) + 5 and t["n_alpn"] == len(alpn or [])
    seen = set()
    for cut in range(len(p)):
        u = TLS.locate(p[:cut])
        if u is None:
            continue
        assert u["flags"] & TLS.TRUNCATED and u["n_ext"] <= t["n_ext"]
        for f in ("sni", "alpn"):
            assert u[f] is None or u[f] == t[f]
        assert all(u[f] == t[f] for f in ("record_version", "client_version", "sid_len", "n_suites", "hs_len"))
        seen.add((u["sni"] is not None, u["alpn"] is not None))
    return seen


def be16(p, i):
    return struct.unpack_from(">H", p, i)[0]


def test_golden_hellos_and_every_prefix():
    hellos = golden_hellos()
    assert len(hellos) == 16
    assert {h["max_version"] for h in hellos} == {"1.2", "1.3"}
    assert any(h["sni"] is None for h in hellos) and any(h["alpn"] is None for h in hellos)
    assert {len(h["sni"]) for h in hellos if h["sni"]} >= {3, 16, 72}
    seen = set()
    for h in hellos:
        seen |= check_hello_and_prefixes(bytes.fromhex(h["hex"]), h["sni"], h["alpn"])
    assert seen == {(False, False), (True, False), (True, True), (False, True)}


def test_fresh_hellos_from_this_interpreter():
    """the generator's own recipe, run now: the model must find what was asked for in whatever this OpenSSL writes"""
    spec = importlib.util.spec_from_file_location("make_tls_goldens", os.path.join(GOLDEN_DIR, "make_tls_goldens.py"))
    gen = importlib.util.module_from_spec(spec)
    try:
        spec.loader.exec_module(gen)
        made = [(gen.client_hello(v, host, alpn), host, alpn) for v, host, alpn in gen.CASES]
    except (ImportError, AttributeError, ValueError, OSError) as e:       # (ssl.SSLError is an OSError)
        pytest.skip(f"this interpreter's ssl cannot write the hellos: {e}")
    for p, host, alpn in made:
        check_hello_and_prefixes(p, host, alpn)


def test_random_payloads_are_none():
    import numpy as np
    rng = np.random.default_rng(7)
    hdr = bytes.fromhex(golden_hellos()[0]["hex"])[:11]
    for k in range(20000):
        p = bytearray(rng.integers(0, 256, int(rng.integers(0, 300)), dtype=np.uint8).tobytes())
        if k % 10 < 7 and len(p) >= 11:
            for i in (0, 1, 2, 5, 9):
                p[i] = hdr[i]
            p[3:5] = b"\xff\xff"
        assert TLS.locate(bytes(p)) is None, bytes(p).hex()
