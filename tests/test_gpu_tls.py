"""kmpgpu_tls_locate / kmpgpu_load_tls (GpuMatcher.tls_locate, .tls_spans, .load_tls) on a real MI355X: the ClientHello in every payload
located on the device, and its server name or its ALPN list as a packed arena that a second context owns, compared with
tests/tls_model.py exactly -- span records, arena bytes including the zero padding, offsets, lengths, the present bitmap with the bits
at n and above 0, the stats, the index and the launches.

Where the kernels of csrc/kmp_tls.hip take another path:
  the golden hellos, and every prefix of one of them as one arena                                     test_golden_hellos, test_every_prefix
  sid 0 .. 32 with names of 0, 1, 15, 16, 17 and 255 bytes (every alignment of the name, across unit borders); ALPN lists of 2, 256 and
  257 bytes and of one name; both orders, behind 40 other extensions; a duplicate server_name; a 256th extension; every malformed
  shape of the definition off by one; arenas of 1, 63, 64, 65 and 129 payloads with hellos and other payloads in one wavefront
                                                                                                      cases(), test_cases
  borrowed arenas whose padding and next slot hold the rest of a cut hello, or a whole hello behind a payload that is none, under both
  settings of whole payloads                                                                          test_dirty_padding
Past the grid caps: tests/test_gpu_tls_scale.py.  The command lines: tests/test_tls_cli.py.

No test provokes a fault: every negative case is one the library refuses on the host before it launches anything.

Run on a real MI355X:  python -m pytest tests/test_gpu_tls.py -m gpu
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
import match_model as MM  # noqa: E402
import tls_model as TLS  # noqa: E402
import multithreading_string_matching_amd as K  # noqa: E402
from multithreading_string_matching_amd import _lib  # noqa: E402
from multithreading_string_matching_amd.host import META_DTYPE  # noqa: E402
from multithreading_string_matching_amd.matcher import (  # noqa: E402
    OPT_NONTEMPORAL, OPT_WHOLE_PAYLOAD, TLS_ALPN, TLS_ALPN_SKIPPED, TLS_CLIENT_HELLO, TLS_FIELD_NAMES, TLS_HAS_ALPN, TLS_HAS_SNI, TLS_NONE,
    TLS_ONLY_PRESENT, TLS_SNI, TLS_SPAN_DTYPE, TLS_TRUNCATED, GpuMatcher)

EINVAL, ESTATE = -2, -3
ONES = 0xFFFFFFFFFFFFFFFF
LAUNCHES = 5                      # kmpgpu.h: field lengths, two scan kernels, index, gather
LAUNCHES_EMPTY = 3                # ... and where dst ends up without a payload; one more where the locate ran
EMPTY = (np.zeros(0, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint32))
GOLDEN = os.path.join(os.path.dirname(DATA), "tls_hellos.json")
H, SNI, ALPN, EXT = TLS.hello, TLS.sni_ext, TLS.alpn_ext, TLS.ext
FIELDS = ("sni", "alpn")


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


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return [bytes.fromhex(h["hex"]) for h in json.load(f)["hellos"]]


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


def check_spans(m, payloads, fresh=True):
    """tls_locate and the records it keeps against the model; fresh: the spans are stale, so the kernel runs"""
    stats = m.tls_locate()
    assert m.last_timing().launches == (1 if fresh and payloads else 0)
    assert stats == TLS.locate_stats(payloads)
    got, want = m.tls_spans(), TLS.spans(payloads)
    assert got.dtype == TLS_SPAN_DTYPE == TLS.SPAN_DTYPE
    if got.tobytes() != want.tobytes():
        k = next(i for i in range(len(payloads)) if got[i].tobytes() != want[i].tobytes())
        raise AssertionError(f"payload {k} ({payloads[k][:60]!r}, length {len(payloads[k])}): {got[k]}, not {want[k]}")


def field_and_check(dst, src, payloads, field, only_present=False, located=False):
    """located: this call has to make the spans first"""
    want = TLS.load_tls(payloads, field, only_present)
    res = dst.load_tls(src, field=field, only_present=only_present)
    assert first_diff(res["present"], want["present"]) is None, first_diff(res["present"], want["present"])
    assert np.array_equal(res["index"], want["index"]) and res["index"].dtype == np.int64
    assert res["stats"] == want["stats"]
    check_arena(dst, want)
    t = dst.last_timing()
    assert t.launches == (LAUNCHES if want["payloads"] else LAUNCHES_EMPTY) + (1 if located else 0) and t.kernel_ms > 0
    return want


def everything(dst, src, payloads):
    """the locate, once more without a launch, and both fields in both modes"""
    check_spans(src, payloads)
    check_spans(src, payloads, fresh=False)
    for field in FIELDS:
        field_and_check(dst, src, payloads, field, False)
        field_and_check(dst, src, payloads, field, True)


def load(m, payloads):
    m.load_arena(K.HostArena.from_payloads(payloads))


# ------------------------------------------------------------------------------------------------
# 1. the golden hellos and the cases of the definition
# ------------------------------------------------------------------------------------------------
def test_golden_hellos(src, dst, golden):
    try:
        reset(src, dst)
        load(src, golden)
        everything(dst, src, golden)
        st = src.tls_locate()
        assert st["n_hellos"] == 16 and st["n_truncated"] == 0 and 0 < st["n_sni"] < 16 and 0 < st["n_alpn"] < 16
    finally:
        reset(src, dst)


def test_every_prefix(src, dst, golden):
    """every prefix of one golden hello with both fields, as one arena: NONE or TRUNCATED, the fields absent or the full hello's"""
    p = golden[0]
    assert len(p) == 517 and TLS.locate(p)["flags"] == TLS.HAS_SNI | TLS.HAS_ALPN
    payloads = [p[:cut] for cut in range(len(p) + 1)]
    flags = {TLS.locate(t)["flags"] for t in payloads if TLS.locate(t)}
    assert flags == {TLS.TRUNCATED, TLS.TRUNCATED | TLS.HAS_SNI, TLS.TRUNCATED | TLS.HAS_SNI | TLS.HAS_ALPN, TLS.HAS_SNI | TLS.HAS_ALPN}
    try:
        reset(src, dst)
        load(src, payloads)
        everything(dst, src, payloads)
    finally:
        reset(src, dst)


def lab(n, salt=0):
    return bytes(0x61 + (i + salt) % 26 for i in range(n))


def cases():
    out = []
    # sid 0 .. 32 moves the name through every alignment; the lengths end in front of, at and behind a unit's border
    for sid in range(33):
        for nl in (0, 1, 15, 16, 17, 255):
            if nl in (15, 16, 17) or sid % 8 == nl % 8:
                out.append(H([SNI(lab(nl, sid)), ALPN([b"h2", b"http/1.1"])], sid=sid))
    assert {TLS.locate(p)["sni_off"] % 16 for p in out} == set(range(16)) and {TLS.locate(p)["sni_len"] for p in out} == {0, 1, 15, 16, 17, 255}
    # ALPN lists of 2, 256 and 257 bytes, one name, many names
    out += [H([ALPN([b"x"])]), H([ALPN([lab(127), lab(127, 3)]), SNI(b"a.b")]), H([ALPN([lab(127), lab(128, 3)]), SNI(b"a.b")]),
            H([ALPN([lab(255, 5)])]), H([ALPN([b"x"] * 128)], sid=7), H([ALPN([lab(1 + i % 9, i) for i in range(40)])], sid=3),
            H([ALPN([0] * 300), SNI(b"skipped.example")])]
    assert [TLS.locate(p)["alpn_len"] for p in out[-7:]] == [1, 255, 0, 255, 255, 229, 0]
    assert TLS.locate(out[-1])["flags"] == TLS.ALPN_SKIPPED | TLS.HAS_SNI
    # both orders, and behind 40 others; a duplicate server_name; no extensions at all
    many = [EXT(100 + i, lab(i % 23, i)) for i in range(40)]
    out += [H([ALPN([b"h2"]), SNI(b"order.example")]), H([SNI(b"order.example"), ALPN([b"h2"])]), H(many + [SNI(b"far.example"), ALPN([b"h3", b"h2"])]),
            H(many + [ALPN([b"h3", b"h2"]), EXT(21, bytes(300)), SNI(b"far.example")], sid=5), H([SNI(b"first.example"), SNI(b"second.example")]),
            H([ALPN([b"h2"]), ALPN([b"h3"]), EXT(0, b"\xff"), EXT(16, b"")]), H(no_ext_block=True), H([]), H(no_ext_block=True, tail=lab(40))]
    # 255 extensions count, a 256th does not
    out += [H([EXT(100 + i, b"") for i in range(254)] + [SNI(b"last.example")]), H([EXT(100 + i, b"") for i in range(255)] + [SNI(b"late.example")])]
    assert TLS.locate(out[-2])["n_ext"] == 255 and TLS.locate(out[-1]) is None
    # every malformed shape, off by one, next to the one that passes
    good = H([SNI(b"example.com"), ALPN([b"h2"])])
    bad = [bytes([21]) + good[1:], good[:1] + b"\x02" + good[2:], good[:2] + b"\x05" + good[3:], good[:5] + b"\x02" + good[6:], good[:9] + b"\x02" + good[10:],
           H([SNI(b"example.com")], rec=len(H([SNI(b"example.com")])) - 9 + 3), good[:44], H(hs=35), H([SNI(b"a.b")], sid=32, sid_byte=33),
           H(suites=0), H(suites=2, cs=3), H(cm=b""), H([SNI(b"a.b")], xlen=len(SNI(b"a.b")) - 1), H([SNI(b"a.b")], xlen=len(SNI(b"a.b")) + 1),
           H([EXT(10, b"xy", n=3)]), H([EXT(10, b"xy"), b"\x00\x00\x00"]), H([EXT(10, b"xy"), EXT(11, b"abcdef", n=7)])[:-3],
           H([EXT(0, b"\x00\x02\x00\x00")]), H([SNI(b"example.com", ll=15)]), H([SNI(b"example.com", name_type=1)]), H([SNI(b"example.com", nl=12)]),
           H([EXT(16, b"\x00\x01\x00")]), H([ALPN([b"h2"], ll=2)]), H([ALPN([b"h2"], ll=4)]), H([EXT(16, b"\x00\x01\x01x")]), H([ALPN([b"h2", 0])]),
           H([ALPN([0, b"h2"])]), H([EXT(16, b"\x00\x05\x02h2\x02x")]), H([SNI(b"ok.example"), ALPN([b"h2", 0])])]
    assert all(TLS.locate(p) is None for p in bad), [i for i, p in enumerate(bad) if TLS.locate(p) is not None]
    ok = [good, H([SNI(b"example.com")], rec=len(H([SNI(b"example.com")])) - 9 + 4), H([EXT(0, b"\x00\x03\x00\x00\x00")]), H([SNI(b"example.com", ll=14)]),
          H([SNI(b"example.com", nl=11)]), H([EXT(16, b"\x00\x02\x01x")]), H([EXT(16, b"\x00\x05\x02h2\x01x")]), H([SNI(b"a.b")], sid=32), H(suites=1),
          H(cm=b"\x01\x00")]
    assert all(TLS.locate(p) is not None for p in ok)
    out += bad + ok
    # cut hellos and what is no hello at all
    out += [good[:-1], good[:len(good) - len(ALPN([b"h2"]))], good[:len(H(no_ext_block=True)) + 2], good[:60], good[:11], good[:10], b"", b"GET / HTTP/1.1\r\n\r\n" + lab(40), bytes(64),
            b"\x16\x03\x01" + b"\xff" * 60, b"\x16\x03\x03\x00\x46\x02\x00\x00\x42\x03\x03" + lab(64)]
    return out


@pytest.mark.parametrize("nontemporal", [1, 0])
def test_cases(src, dst, nontemporal):
    cs = cases()
    kinds = TLS.spans(cs)
    assert {int(k) for k in kinds["kind"]} == {TLS.NONE, TLS.CLIENT_HELLO} and {int(f) for f in kinds["flags"]} >= {0, 1, 2, 3, 4, 5, 9}
    try:
        reset(src, dst)
        dst.set_option(OPT_NONTEMPORAL, nontemporal)
        # all cases at once, then arenas of 1, 63, 64, 65 and 129 payloads: hellos and other payloads share a wavefront
        groups = [cs] + [[cs[(7 * n + 5 * i) % len(cs)] for i in range(n)] for n in (1, 63, 64, 65, 129)]
        for g in groups:
            if 1 < len(g) < len(cs):
                verdicts = [TLS.locate(t) is None for t in g[:64]]
                assert any(verdicts) and not all(verdicts)
            load(src, g)
            everything(dst, src, g)
    finally:
        reset(src, dst)
        src.load_arena(*EMPTY)


def dirty(golden):
    """(payloads, slots) of a borrowed arena: slots[k] is payload k and what lies behind it up to its slot's end"""
    full = [golden[0], golden[4], H([SNI(b"example.com"), ALPN([b"h2", b"http/1.1"])], sid=5), H([ALPN([b"h2"]), SNI(lab(40))], sid=0)]
    payloads, slots = [], []
    for p in full:
        t = TLS.locate(p)
        whole = p + bytes(-len(p) % 16)
        cuts = {11, 16, 43, 44, 48, 64, t["sni_off"] - 5, t["sni_off"], t["sni_off"] + t["sni_len"] - 1, t["sni_off"] + t["sni_len"],
                t["alpn_off"] - 3, t["alpn_off"] + t["alpn_len"] - 1, t["alpn_off"] + t["alpn_len"], len(p) - 17, len(p) - 16, len(p) - 1}
        for L in sorted(c for c in cuts if 0 < c < len(p)):
            # a truncated hello whose padding holds the next bytes of the hello
            payloads.append(p[:L])
            slots.append(whole[:max(16, (L + 15) & ~15)])
            if L % 16 == 0:                                                  # ... and whose next slot begins with what would continue it
                payloads.append(p[L:L + 24])
                slots.append((p[L:] + bytes(32))[:32])
        # a payload that is no hello, whose slot holds a whole one
        for L in (0, 1, 5, 10):
            payloads.append(p[:L])
            slots.append(whole)
    assert all(len(s) % 16 == 0 and len(s) >= max(16, len(t)) and s[:len(t)] == t for t, s in zip(payloads, slots))
    return payloads, slots


@pytest.mark.parametrize("whole", [0, 1])
def test_dirty_padding(src, dst, whole, golden):
    """a borrowed arena keeps what lies behind L: the rest of a cut hello must not complete it, a hello behind a payload that is none
    must not be found"""
    payloads, slots = dirty(golden)
    # reading behind L would change the verdict: the model decides otherwise over the slot's bytes
    flipped = sum(TLS.span(t) != TLS.span(s) for t, s in zip(payloads, slots))
    none_to_hello = sum(TLS.locate(t) is None and TLS.locate(s) is not None for t, s in zip(payloads, slots))
    assert flipped >= 20 and none_to_hello == 16, (flipped, none_to_hello)
    assert sum(bool(TLS.locate(t) and TLS.locate(t)["flags"] & TLS.TRUNCATED) for t in payloads) >= 20
    try:
        reset(src, dst)
        src.set_option(OPT_WHOLE_PAYLOAD, whole)
        dst.set_option(OPT_WHOLE_PAYLOAD, whole)
        keep = attach_slots(src, payloads, slots)
        everything(dst, src, payloads)
        del keep
    finally:
        reset(src, dst)
        src.load_arena(*EMPTY)


# ------------------------------------------------------------------------------------------------
# 2. outcomes, metadata, the cache, the source, the errors
# ------------------------------------------------------------------------------------------------
def mixed(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        if k % 4 == 3:
            out.append(rng.integers(0, 256, int(rng.integers(0, 90)), dtype=np.uint8).tobytes())
        else:
            exts = [EXT(100 + i, lab(int(rng.integers(0, 20)), i)) for i in range(int(rng.integers(0, 5)))]
            if k % 3 != 2:
                exts.insert(int(rng.integers(0, len(exts) + 1)), SNI(lab(int(rng.integers(0, 60)), k)))
            if k % 5 != 4:
                exts.insert(int(rng.integers(0, len(exts) + 1)), ALPN([lab(int(rng.integers(1, 12)), k + i) for i in range(int(rng.integers(1, 5)))]))
            p = H(exts, sid=int(rng.integers(0, 33)), suites=int(rng.integers(1, 20)))
            out.append(p[:int(rng.integers(0, len(p)))] if k % 7 == 0 else p)
    return out


def meta_for(n):
    meta = np.zeros(n, dtype=META_DTYPE)
    meta["src_ip"], meta["dst_ip"] = 0x0A000001 + np.arange(n), 0xC0A80101
    meta["src_port"], meta["dst_port"], meta["proto"] = 40000 + np.arange(n) % 1000, np.where(np.arange(n) % 3 == 0, 8443, 443), 6
    return meta


def test_arena_outcomes_and_metadata(src, dst):
    g = _lib.gpu_lib()
    a = H([SNI(b"example.com"), ALPN([b"h2", b"http/1.1"])])
    msgs = [a, b"no tls", H([SNI(b"")]), b"", H([ALPN([b"h2"])]), a[:-3]]
    meta = meta_for(len(msgs))
    try:
        reset(src, dst)
        load(src, msgs)
        src.set_meta(meta)
        want = field_and_check(dst, src, msgs, "sni", only_present=True, located=True)
        assert want["payloads"] == [b"example.com", b"", b"example.com"] and want["index"].tolist() == [0, 2, 5]
        assert dst.meta().tobytes() == meta[[0, 2, 5]].tobytes()
        want = field_and_check(dst, src, msgs, "alpn", only_present=True)
        assert want["payloads"] == [b"h2,http/1.1", b"h2"] and dst.meta().tobytes() == meta[[0, 4]].tobytes()
        field_and_check(dst, src, msgs, "alpn")
        assert dst.meta().tobytes() == meta.tobytes()
        # no payload has the field: dst without an arena, three launches and the locate
        none = [b"tls", b"", bytes(40), H([EXT(10, b"xy")]), H(no_ext_block=True)]
        load(src, none)
        field_and_check(dst, src, none, "sni", only_present=True, located=True)
        assert dst.arena_info() == (0, 0)
        field_and_check(dst, src, none, "alpn", only_present=False)
        assert dst.arena_info() == (5, 0)
        # an empty source
        src.load_arena(*EMPTY)
        st = _lib.FieldsStats()
        d_present = C.c_void_p(1)
        assert g.kmpgpu_load_tls(dst._ctx, src._ctx, TLS_SNI, TLS_ONLY_PRESENT, None, C.byref(d_present), C.byref(st)) == 0
        assert dst.arena_info() == (0, 0) and st.n_payloads == 0 and not d_present.value
        res = dst.load_tls(src, "alpn")
        assert res["present"].shape == (0,) and res["index"].shape == (0,) and res["stats"]["n_payloads"] == 0
        assert src.tls_locate() == {"n_hellos": 0, "n_sni": 0, "n_alpn": 0, "n_truncated": 0} and src.tls_spans().shape == (0,)
    finally:
        reset(src, dst)


def test_spans_life_cycle(src, dst, third):
    """a second locate launches nothing; dropped by every loader (load_selected into the source among them), kept by a scan; read in
    ranges; refused where there are none; the HTTP and DNS spans live beside them"""
    g = _lib.gpu_lib()
    a, b = mixed(150, seed=192), mixed(90, seed=193)
    out = np.zeros(4, dtype=TLS_SPAN_DTYPE)
    try:
        reset(src, dst, third)
        src.set_patterns([lab(3)])
        load(src, a)
        assert g.kmpgpu_tls_spans_read(src._ctx, out.ctypes.data, 0, 1) == ESTATE and b"no spans" in g.kmpgpu_last_error()
        field_and_check(dst, src, a, "sni", located=True)
        assert src.tls_spans().tobytes() == TLS.spans(a).tobytes()
        check_spans(src, a, fresh=False)                                          # a second locate launches 0
        field_and_check(dst, src, a, "alpn")                                      # ... and the other field needs none either
        assert g.kmpgpu_tls_spans_read(src._ctx, out.ctypes.data, 146, 4) == 0 and out.tobytes() == TLS.spans(a[146:]).tobytes()
        assert g.kmpgpu_tls_spans_read(src._ctx, out.ctypes.data, 147, 4) == EINVAL and g.kmpgpu_tls_spans_read(src._ctx, None, 0, 1) == EINVAL
        assert g.kmpgpu_tls_spans_read(None, out.ctypes.data, 0, 1) == EINVAL and g.kmpgpu_tls_locate(None, 0, None) == EINVAL
        assert g.kmpgpu_tls_locate(src._ctx, 1, None) == EINVAL and b"flag bits" in g.kmpgpu_last_error()
        src.http_locate()                                                         # the HTTP and DNS spans do not touch them
        src.dns_locate()
        src.scan()
        src.scan_packets()
        field_and_check(dst, src, a, "sni", only_present=True)                    # a scan keeps them
        third.load_arena(K.HostArena.from_payloads(b))
        pick = np.arange(len(b)) % 2 == 0
        src.load_selected(third, pick)                                            # load_selected into the source drops them
        assert g.kmpgpu_tls_spans_read(src._ctx, out.ctypes.data, 0, 1) == ESTATE
        kept = [t for t, p in zip(b, pick) if p]
        field_and_check(dst, src, kept, "alpn", located=True)
        check_spans(src, kept, fresh=False)
        assert g.kmpgpu_tls_spans_read(dst._ctx, out.ctypes.data, 0, 1) == ESTATE              # dst's own are not src's
        load(src, b)                                                              # a reload of the arena drops them
        assert g.kmpgpu_tls_spans_read(src._ctx, out.ctypes.data, 0, 1) == ESTATE
        check_spans(src, b)
        # the pairs of the profile: the locate, then lengths, scan, index, gather
        load(src, a)
        dst.profile_begin(8)
        dst.load_tls(src, "alpn")
        ms = dst.profile_end(8)
        assert len(ms) == 5 and (ms >= 0).all()
    finally:
        reset(src, dst, third)
        src.set_patterns([b"x"])


def test_src_untouched(src, dst):
    payloads = mixed(300, seed=194)
    pats = [lab(3), b"\x13\x01", lab(2, 1)]
    try:
        reset(src, dst)
        src.set_patterns(pats)
        src.set_option(OPT_WHOLE_PAYLOAD, 1)
        load(src, payloads)
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
    payloads = mixed(120, seed=195)
    kept = mixed(77, seed=196)
    want_kept = dict(zip(("arena", "off", "len"), DM.packed_image(kept)))
    st = _lib.FieldsStats()
    d_present = C.c_void_p()
    words = np.zeros(8, dtype=np.uint64)

    def call(d, s, field=TLS_SNI, flags=0):
        st.n_payloads = 12345
        d_present.value = 1
        return g.kmpgpu_load_tls(d, s, field, flags, words.ctypes.data, C.byref(d_present), C.byref(st))

    def dst_keeps_its_arena(rc, code, what):
        assert rc == code, (rc, code)
        msg = g.kmpgpu_last_error()
        assert b"kmpgpu_load_tls" in msg and what in msg, msg
        assert st.n_payloads == 0 and not d_present.value
        check_arena(dst, want_kept)

    try:
        reset(src, dst)
        load(src, payloads)
        load(dst, kept)
        dst_keeps_its_arena(call(dst._ctx, dst._ctx), EINVAL, b"same context")
        dst_keeps_its_arena(call(None, src._ctx), EINVAL, b"ctx is NULL")
        dst_keeps_its_arena(call(dst._ctx, None), EINVAL, b"ctx is NULL")
        dst_keeps_its_arena(call(dst._ctx, src._ctx, field=0), EINVAL, b"field 0")
        dst_keeps_its_arena(call(dst._ctx, src._ctx, field=3), EINVAL, b"field 3")
        dst_keeps_its_arena(call(dst._ctx, src._ctx, flags=2), EINVAL, b"flag bits")
        dst_keeps_its_arena(call(dst._ctx, src._ctx, flags=0x80000001), EINVAL, b"flag bits")
        assert g.kmpgpu_tls_spans_read(src._ctx, words.ctypes.data, 0, 1) == ESTATE          # none of these made the spans
        with pytest.raises(ValueError):
            dst.load_tls(src, field="ja3")
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
                assert g.kmpgpu_tls_locate(other._ctx, 0, None) == ESTATE and b"kmpgpu_tls_locate" in g.kmpgpu_last_error()
                n_pay = C.c_uint64()
                assert g.kmpgpu_load_frames_finish(other._ctx, C.byref(n_pay)) == 0
        finally:
            _lib.host_lib().kmp_frames_free(C.byref(fr))
        # NULL outputs, and the device words with the bits at n and above 0
        assert g.kmpgpu_load_tls(dst._ctx, src._ctx, TLS_ALPN, 0, None, None, None) == 0
        check_arena(dst, TLS.load_tls(payloads, "alpn"))
        assert dst.last_timing().launches == LAUNCHES + 1
        words[:] = np.uint64(ONES)
        assert call(dst._ctx, src._ctx, flags=TLS_ONLY_PRESENT) == 0 and d_present.value
        have = TLS.load_tls(payloads, "sni", True)
        assert np.array_equal(words[:2], have["words"]) and st.n_payloads == st.n_present == len(have["index"])
    finally:
        reset(src, dst)


# ------------------------------------------------------------------------------------------------
# 3. what the buffers are for
# ------------------------------------------------------------------------------------------------
def test_hello_cut_over_two_segments_is_whole_in_the_stream(src, dst, third, golden):
    """a ClientHello in two TCP segments of one flow: NONE or TRUNCATED on the capture, whole through load_streams and load_tls"""
    p = golden[0]
    cut = TLS.locate(p)["sni_off"] + 4                                 # inside the server name
    payloads = [p[:cut], p[cut:], golden[4], b"\x17\x03\x03\x00\x05hello"]
    meta = np.zeros(4, dtype=META_DTYPE)
    meta["src_ip"], meta["dst_ip"], meta["dst_port"], meta["proto"] = 0x0A000001, 0xC0A80101, 443, 6
    meta["src_port"] = [40001, 40001, 40002, 40002]
    try:
        reset(src, dst, third)
        load(src, payloads)
        src.set_meta(meta)
        check_spans(src, payloads)
        sp = src.tls_spans()
        assert sp["kind"].tolist() == [TLS_CLIENT_HELLO, TLS_NONE, TLS_CLIENT_HELLO, TLS_NONE] and sp["flags"][0] == TLS_TRUNCATED
        assert dst.load_tls(src, "sni")["present"].tolist() == [False, False, True, False]
        src.build_flows()
        n_streams = third.load_streams(src)
        a, off, ln = third.arena_download()
        streams = [a[o:o + l].tobytes() for o, l in zip(off.tolist(), ln.tolist())]
        assert len(streams) == n_streams and p in streams and any(s.startswith(golden[4]) and len(s) > len(golden[4]) for s in streams)
        check_spans(third, streams)
        for field in FIELDS:
            want = field_and_check(dst, third, streams, field, only_present=True)
            assert want["payloads"] == [TLS.locate(p)[field], TLS.locate(golden[4])[field]]
    finally:
        reset(src, dst, third)


def test_rule_of_a_linked_sni_row_and_a_header_predicate(src, dst, golden):
    """alert tcp any any -> any 443 (tls.sni; content:"example.com"): the server-name row comes from the SNI buffer through a link, the
    port from the capture context's metadata; the same bytes elsewhere in a payload do not count"""
    payloads = list(golden) + [b"GET / HTTP/1.1\r\nHost: example.com\r\n\r\n", H([EXT(100, b"example.com")]), H([SNI(b"www.example.com")]),
                               H([SNI(b"example.org")]), H([SNI(b"example.com")])[:-2], b""]
    meta = meta_for(len(payloads))
    sni = [TLS.field_of(t, "sni") or b"" for t in payloads]
    want = np.array([b"example.com" in s for s in sni]) & (meta["dst_port"] == 443)
    raw = np.array([b"example.com" in t for t in payloads])
    assert 0 < want.sum() < sum(b"example.com" in s for s in sni) and (raw & ~np.array([b"example.com" in s for s in sni])).sum() >= 2
    try:
        reset(src, dst)
        load(src, payloads)
        src.set_meta(meta)
        dst.set_patterns([b"example.com"])
        dst.set_rules([([0], [])])
        src.set_patterns([b"unused"])
        src.set_headers([{"dport_lo": 443, "dport_hi": 443, "proto": 6}])
        src.set_links(1)
        src.set_rules([([src.link(0), src.hdr(0)], [])])
        # the identity map: dst holds every payload
        dst.load_tls(src, "sni")
        src.link_rows(0, dst, "rules")
        res = src.scan_rules(hits=True)
        assert np.array_equal(res["hits"][0], want) and res["rule_pkt_counts"].tolist() == [int(want.sum())]
        # the present bitmap: dst holds the payloads with a server name only
        present = dst.load_tls(src, "sni", only_present=True)["present"]
        src.link_rows(0, dst, "rules", map=present)
        res = src.scan_rules(hits=True)
        assert np.array_equal(res["hits"][0], want)
    finally:
        reset(src, dst)
        src.set_links(0)
        src.set_headers(None)
        for m in (src, dst):
            m.set_patterns([b"x"])


def test_constants():
    assert TLS_FIELD_NAMES == {"sni": 1, "alpn": 2} and (TLS_SNI, TLS_ALPN, TLS_ONLY_PRESENT) == (1, 2, 1)
    assert (TLS_NONE, TLS_CLIENT_HELLO) == (TLS.NONE, TLS.CLIENT_HELLO) == (0, 1)
    assert (TLS_HAS_SNI, TLS_HAS_ALPN, TLS_TRUNCATED, TLS_ALPN_SKIPPED) == (TLS.HAS_SNI, TLS.HAS_ALPN, TLS.TRUNCATED, TLS.ALPN_SKIPPED) == (1, 2, 4, 8)
    assert (K.TLS_SNI, K.TLS_ALPN, K.TLS_ONLY_PRESENT) == (1, 2, 1)
