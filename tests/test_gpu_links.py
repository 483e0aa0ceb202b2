"""Linked rows (kmpgpu_set_links, kmpgpu_link_rows, kmpgpu_scan_links): a row another context computed over its own view of the payloads
as a row and rule term of this context, against tests/link_model.py and against the route a caller had to take before -- every context
scanned with hits=True and the rows combined with numpy.  Every comparison is exact."""
import contextlib
import ctypes as C
import os
import re

import numpy as np
import pytest

from gpu_support import reset, torch  # noqa: F401  (before the package: gpu_support says why)

import decode_model as DM
import flow_model as FM
import http_model as HM
import link_model as LM
import match_model as MM
from multithreading_string_matching_amd import _lib
from multithreading_string_matching_amd.host import META_DTYPE, HostArena
from multithreading_string_matching_amd.matcher import (DECODE_ONLY_CHANGED, DECODE_PERCENT, LINK_BITMAP, LINK_INDEX, LINK_NONE, LINK_SAME,
                                                        GpuMatcher)

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -2, -3
ONES = 0xFFFFFFFFFFFFFFFF
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "multithreading_string_matching_amd", "csrc", "kmp_launch.h")) as _f:
    RANK_TILE = int(re.search(r"#define KMP_LINK_RANK_TILE (\d+)u", _f.read()).group(1))      # map words per block of the rank kernel


@contextlib.contextmanager
def matchers(*pattern_sets):
    ms = []
    try:
        for pats in pattern_sets:
            m = GpuMatcher(0)
            m.set_patterns(list(pats))
            ms.append(m)
        yield ms
    finally:
        for m in ms:
            m.close()


@contextlib.contextmanager
def raises(code, text):
    with pytest.raises(_lib.KmpGpuError) as e:
        yield
    assert f"({code})" in str(e.value) and text in str(e.value), str(e.value)


def raw_link(dst, first_link, src, family, first_row, n_rows, kind, ptr, on_device):
    return dst._g.kmpgpu_link_rows(dst._ctx, first_link, src._ctx if src is not None else None, family, first_row, n_rows, kind, ptr, on_device, None)


def link_words(m):
    """the link rows as the library hands them out, every word of them, into buffers that start as all ones"""
    n, _ = m.arena_info()
    W = (n + 63) // 64
    hit_w, any_w = np.full((m.n_links, W), ONES, dtype=np.uint64), np.full(W, ONES, dtype=np.uint64)
    pc = np.zeros(m.n_links, dtype=np.uint64)
    _lib.gpu_check(m._g.kmpgpu_scan_links(m._ctx, pc.ctypes.data, any_w.ctypes.data, hit_w.ctypes.data, None, None), "kmpgpu_scan_links")
    return hit_w, any_w, pc


def check_links(m, want):
    """scan_links against bool[n_links, n]: the rows, their counts, their OR, and the raw words (bits at n and above are 0)"""
    res = m.scan_links(hits=True)
    bad = np.argwhere(res["hits"] != want)
    assert bad.size == 0, [(int(q), int(k), bool(want[q, k])) for q, k in bad[:8]]
    assert res["link_pkt_counts"].tolist() == want.sum(axis=1).tolist()
    assert res["any"].tolist() == want.any(axis=0).tolist()
    hit_w, any_w, pc = link_words(m)
    assert np.array_equal(hit_w, MM.words(want)) and np.array_equal(any_w, MM.words(want.any(axis=0)))
    assert pc.tolist() == want.sum(axis=1).tolist()


def text_payloads(n, n_rows, seed):
    """n payloads and n_rows patterns "<Rq>": payload k holds pattern q where the returned bool[n_rows, n] says so"""
    rng = np.random.default_rng(seed)
    want = rng.random((n_rows, n)) < 0.4
    want[:, -1] = True                                 # the last payload, the last bit of the tail word
    pats = [b"<R%d>" % q for q in range(n_rows)]
    pay = [b"pad " + b"".join(pats[q] for q in range(n_rows) if want[q, k]) + b" end" for k in range(n)]
    return pay, pats, want


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. end to end: one rule over three buffers and the header
# ------------------------------------------------------------------------------------------------------------------------------------
def http_capture():
    """208 hand-made payloads: every combination of where "/admin" stands (plain in the URI, percent-encoded in the URI, only in the
    body, nowhere), where "evil" stands (body, a header, nowhere) and which Host the headers name, on port 80 or 8080, plus payloads that
    are no HTTP at all.  13 clients, each talking to both ports: 26 flows."""
    uris = [b"/admin/panel", b"/%61dm%69n?x=1", b"/index.html", b"/adm%2Fin"]
    bodies = [b"an evil payload", b"harmless /admin text", b""]
    hosts = [b"Host: intranet.corp", b"Host: example.org", b"Host: example.org\r\nX-Note: evil"]
    pay, meta = [], []
    k = 0
    for rep in range(3):
        for u in uris:
            for b in bodies:
                for h in hosts:
                    for port in (80, 8080):
                        if rep == 2 and port == 8080:
                            continue
                        pay.append(b"POST " + u + b" HTTP/1.1\r\n" + h + b"\r\nContent-Length: %d\r\n\r\n" % len(b) + b)
                        meta.append((0x0A000001 + k % 13, 0xC0A80101, 1024 + k % 13, port))
                        k += 1
    for junk in (b"", b"evil /admin intranet", b"\x00\x01\x02", b"GET"):
        for port in (80, 8080):
            pay.append(junk)
            meta.append((0x0A000001 + k % 13, 0xC0A80101, 1024 + k % 13, port))
            k += 1
    m = np.zeros(len(pay), dtype=META_DTYPE)
    for r, (s, d, sp, dp) in zip(m, meta):
        r["src_ip"], r["dst_ip"], r["src_port"], r["dst_port"], r["proto"] = s, d, sp, dp, 6
    return pay, m


@pytest.fixture(scope="module")
def three_buffers():
    """the capture's context with the rule over three links and a header predicate, the four derived contexts, and the verdict worked
    out from the models of the fields and the decoding"""
    pay, meta = http_capture()
    n = len(pay)
    with matchers([b"unused"], [b"unused"], [b"/admin"], [b"evil"], [b"intranet"]) as (cap, uri, dec, body, hdrs):
        arena = HostArena.from_payloads(pay)
        cap.load_arena(arena)
        cap.set_meta(meta)
        cap.set_headers([{"dport_lo": 80, "dport_hi": 80}])
        cap.set_links(3)
        cap.set_rules([([cap.link(0), cap.link(1), cap.hdr(0)], [cap.link(2)])])
        uri.load_fields(cap, "raw_uri")
        dec.load_decoded(uri)
        body.load_fields(cap, "body")
        hdrs.load_fields(cap, "headers")
        model = {"admin": np.array([b"/admin" in DM.decode(HM.field(p, "raw_uri") or b"").split(b"\0")[0] for p in pay]),
                 "evil": np.array([b"evil" in (HM.field(p, "body") or b"").split(b"\0")[0] for p in pay]),
                 "intranet": np.array([b"intranet" in (HM.field(p, "headers") or b"").split(b"\0")[0] for p in pay]),
                 "port": meta["dst_port"] == 80}
        yield {"n": n, "pay": pay, "meta": meta, "cap": cap, "dec": dec, "body": body, "hdrs": hdrs, "model": model}


def fill_three(tb):
    cap = tb["cap"]
    cap.link_rows(0, tb["dec"], "patterns")
    cap.link_rows(1, tb["body"], "patterns")
    cap.link_rows(2, tb["hdrs"], "patterns")


def test_rule_over_three_buffers_equals_the_host_route(three_buffers):
    tb = three_buffers
    cap, mo = tb["cap"], tb["model"]
    fill_three(tb)
    got = cap.scan_rules(hits=True)
    # the route a caller had to take: every context's rows downloaded, combined on the host
    a = tb["dec"].scan_packets(hits=True)["hits"][0]
    e = tb["body"].scan_packets(hits=True)["hits"][0]
    i = tb["hdrs"].scan_packets(hits=True)["hits"][0]
    p = cap.scan_headers(hits=True)["hits"][0]
    host = a & e & ~i & p
    assert np.array_equal(got["hits"][0], host)
    assert got["rule_pkt_counts"].tolist() == [int(host.sum())] and np.array_equal(got["any"], host)
    # ... and both are what the models of the fields and of the decoding say, which is neither nothing nor everything
    want = mo["admin"] & mo["evil"] & ~mo["intranet"] & mo["port"]
    assert 0 < want.sum() < mo["admin"].sum() and np.array_equal(host, want)
    assert np.array_equal(a, mo["admin"]) and np.array_equal(e, mo["evil"]) and np.array_equal(i, mo["intranet"])
    check_links(cap, np.stack([a, e, i]))


def test_the_verdict_reaches_the_alert_list_and_the_flows(three_buffers):
    tb = three_buffers
    cap, mo = tb["cap"], tb["model"]
    fill_three(tb)
    want = mo["admin"] & mo["evil"] & ~mo["intranet"] & mo["port"]
    al = cap.scan_alerts("rules")
    assert al["n_found"] == int(want.sum()) and al["alerts"]["packet"].tolist() == np.flatnonzero(want).tolist()
    assert set(al["alerts"]["index"].tolist()) == {0}
    fo = FM.flow_of(tb["meta"])
    assert cap.build_flows() == int(fo.max()) + 1 == 26
    terms = np.stack([mo["admin"], mo["evil"], mo["intranet"], mo["port"]])
    per_flow = FM.flow_rules(terms, fo, [([0, 1, 3], [2])])
    res = cap.scan_flows("rules", "flow", hits=True)
    assert np.array_equal(res["hits"], per_flow)
    assert np.array_equal(cap.scan_flows("rules", "packet", hits=True)["hits"], FM.fold(want[None, :], fo))


# ------------------------------------------------------------------------------------------------------------------------------------
# 2. SAME
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rows", [1, 2, 65])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 128, 129])
def test_same(n, n_rows):
    pay, pats, want = text_payloads(n, n_rows, seed=n * 100 + n_rows)
    with matchers([b"unused"], pats) as (dst, src):
        dst.load_arena(HostArena.from_payloads([b"x"] * n))
        src.load_arena(HostArena.from_payloads(pay))
        dst.set_links(n_rows + 1)                      # one link more than is filled: it stays all zero
        dst.link_rows(1, src, "patterns")
        model = np.concatenate([np.zeros((1, n), bool), LM.link(want, n, n, LM.SAME)])
        check_links(dst, model)
        # one row of the family, by number, into the link left out
        dst.link_rows(0, src, "patterns", rows=n_rows - 1)
        model[0] = want[n_rows - 1]
        check_links(dst, model)


# ------------------------------------------------------------------------------------------------------------------------------------
# 3. BITMAP
# ------------------------------------------------------------------------------------------------------------------------------------
def decoded_only_changed(dec, src):
    """kmpgpu_load_decoded(only_changed) with both forms of the changed bitmap: (host words, device pointer)"""
    n, _ = src.arena_info()
    words = np.zeros(max((n + 63) // 64, 1), dtype=np.uint64)
    d_ptr = C.c_void_p()
    st = _lib.DecodeStats()
    _lib.gpu_check(dec._g.kmpgpu_load_decoded(dec._ctx, src._ctx, DECODE_PERCENT, DECODE_ONLY_CHANGED, words.ctypes.data, C.byref(d_ptr),
                                              C.byref(st)), "kmpgpu_load_decoded")
    return words[:(n + 63) // 64], d_ptr


def escaped_payloads(n, changed, seed):
    """payload k holds "<HIT>" where the returned bool[n] says so -- percent-encoded where `changed` asks for a payload the decoding
    changes, plain elsewhere"""
    rng = np.random.default_rng(seed)
    hit = rng.random(n) < 0.5
    hit[-1] = True
    pay = []
    for k in range(n):
        t = b"k%d " % k + (b"<HIT>" if hit[k] else b"<MISS>")
        pay.append(t.replace(b"<", b"%3C") if changed[k] else t)
    return pay, hit


CHANGED = {"none": lambda n: np.zeros(n, bool), "all": lambda n: np.ones(n, bool), "alternating": lambda n: np.arange(n) % 2 == 1,
           "last": lambda n: np.arange(n) == n - 1}


@pytest.mark.parametrize("shape", sorted(CHANGED))
@pytest.mark.parametrize("n", [130, RANK_TILE * 64 - 1, RANK_TILE * 64, RANK_TILE * 64 + 1])
def test_bitmap_from_the_changed_payloads(n, shape):
    changed = CHANGED[shape](n)
    pay, hit = escaped_payloads(n, changed, seed=n)
    with matchers([b"unused"], [b"<HIT>", b"k"]) as (cap, dec):
        cap.load_arena(HostArena.from_payloads(pay))
        words, d_ptr = decoded_only_changed(dec, cap)
        assert np.array_equal(words, MM.words(changed))
        n_src = int(changed.sum())
        src_rows = np.stack([hit[changed], np.ones(n_src, bool)])
        want = LM.link(src_rows, n_src, n, LM.BITMAP, changed)
        assert np.array_equal(want, np.stack([hit & changed, changed]))
        cap.set_links(4)
        # the device pointer as the loader hands it out, and the host words
        assert raw_link(cap, 0, dec, 0, 0, 2, LINK_BITMAP, d_ptr, 1) == 0
        cap.link_rows(2, dec, "patterns", map=words)
        check_links(cap, np.concatenate([want, want]))
        # garbage at n and above names no payload
        if n % 64:
            dirty = words.copy()
            dirty[-1] |= np.uint64(ONES) << np.uint64(n % 64)
            cap.link_rows(0, dec, "patterns", map=dirty)
            dev = torch.from_numpy(dirty.view(np.int64)).cuda()
            cap.link_rows(2, dec, "patterns", map=dev)
            check_links(cap, np.concatenate([want, want]))
        # a bool array is packed on the way
        cap.set_links(2)
        cap.link_rows(0, dec, "patterns", map=changed)
        check_links(cap, want)


def test_bitmap_popcount_mismatch_leaves_the_links_alone():
    n = 200
    changed = CHANGED["alternating"](n)
    pay, hit = escaped_payloads(n, changed, seed=7)
    with matchers([b"unused"], [b"<HIT>"]) as (cap, dec):
        cap.load_arena(HostArena.from_payloads(pay))
        words, d_ptr = decoded_only_changed(dec, cap)
        cap.set_links(1)
        cap.link_rows(0, dec, "patterns", map=words)
        want = (hit & changed)[None, :]
        check_links(cap, want)
        for flip in (0, n - 1):                        # one bit more, one bit fewer
            bad = words.copy()
            bad[flip // 64] ^= np.uint64(1) << np.uint64(flip % 64)
            with raises(EINVAL, "bits set below"):
                cap.link_rows(0, dec, "patterns", map=bad)
            check_links(cap, want)
        # a bit at n or above does not count
        ok = words.copy()
        ok[-1] |= np.uint64(1) << np.uint64(63)
        cap.link_rows(0, dec, "patterns", map=ok)
        check_links(cap, want)


# ------------------------------------------------------------------------------------------------------------------------------------
# 4. INDEX
# ------------------------------------------------------------------------------------------------------------------------------------
def test_index_from_the_stream_map():
    """a content split over two segments is found in the stream context only, and reaches both payloads of the stream"""
    pay = [b"first half SPL", b"IT second half", b"nothing here", b"SPLIT in one piece", b"other flow SPL", b"unrelated"]
    flow = [0, 0, 1, 1, 2, 3]
    meta = np.zeros(len(pay), dtype=META_DTYPE)
    for r, f in zip(meta, flow):
        r["src_ip"], r["dst_ip"], r["src_port"], r["dst_port"], r["proto"] = 0x0A000001 + f, 0xC0A80101, 1000 + f, 80, 6
    with matchers([b"SPLIT"], [b"SPLIT"]) as (cap, st):
        cap.load_arena(HostArena.from_payloads(pay))
        cap.set_meta(meta)
        cap.build_flows()
        n_streams = st.load_streams(cap)
        smap = st.stream_map()["stream"].astype(np.uint32)
        assert n_streams == 4 and smap[0] == smap[1] and smap[2] == smap[3] and len(set(smap.tolist())) == 4
        in_stream = st.scan_packets(hits=True)["hits"]
        own = cap.scan_packets(hits=True)["hits"][0]
        assert own.tolist() == [False, False, False, True, False, False]
        cap.set_links(1)
        cap.link_rows(0, st, "patterns", map=smap)
        want = LM.link(in_stream, n_streams, len(pay), LM.INDEX, smap)
        assert want[0].tolist() == [True, True, True, True, False, False]
        check_links(cap, want)
        # NONE and an index equal to n_src both read as no bit; the rest stays
        holes = smap.copy()
        holes[0], holes[3] = LINK_NONE, n_streams
        cap.link_rows(0, st, "patterns", map=holes)
        want = LM.link(in_stream, n_streams, len(pay), LM.INDEX, holes)
        assert want[0].tolist() == [False, True, True, False, False, False]
        check_links(cap, want)
        dev = torch.from_numpy(holes.view(np.int32)).cuda()
        cap.link_rows(0, st, "patterns", map=dev)
        check_links(cap, want)
        # a rule over the link and a pattern of the capture's own
        cap.set_rules([([cap.link(0)], [0])])
        assert cap.scan_rules(hits=True)["hits"][0].tolist() == [False, True, True, False, False, False]


# ------------------------------------------------------------------------------------------------------------------------------------
# 5. chaining: capture <- raw_uri <- decoded
# ------------------------------------------------------------------------------------------------------------------------------------
def test_links_chain_through_three_contexts():
    uris = [b"/%61dmin", b"/admin", b"/plain", b"/%70lain", b"/ad%6Din/x"]
    pay = []
    for k in range(150):
        pay.append(b"GET " + uris[k % 5] + b" HTTP/1.1\r\nHost: h\r\n\r\n" if k % 7 else b"no http %d" % k)
    with matchers([b"unused"], [b"/"], [b"/admin"]) as (cap, uri, dec):
        cap.load_arena(HostArena.from_payloads(pay))
        present = uri.load_fields(cap, "raw_uri", only_present=True)["present"]
        changed = dec.load_decoded(uri, only_changed=True)["changed"]
        verdict = dec.scan_packets(hits=True)["hits"]
        # decoded -> raw_uri: a link of uri, exposed as a single-term rule of uri
        uri.set_links(1)
        uri.link_rows(0, dec, "patterns", map=changed)
        uri.set_rules([([uri.link(0)], []), ([0], [uri.link(0)])])
        mid = LM.link(verdict, int(changed.sum()), int(present.sum()), LM.BITMAP, changed)
        assert np.array_equal(uri.scan_rules(hits=True)["hits"][0], mid[0])
        # raw_uri -> capture: src's family is its rules, whose terms name src's own link
        cap.set_links(2)
        cap.link_rows(0, uri, "rules", map=present)
        top = LM.link(mid, int(present.sum()), len(pay), LM.BITMAP, present)
        want = np.array([(k % 7 != 0) and (k % 5 in (0, 4)) for k in range(len(pay))])
        assert np.array_equal(top[0], want)
        check_links(cap, np.stack([want, present & ~want]))


# ------------------------------------------------------------------------------------------------------------------------------------
# 6. state and refusals
# ------------------------------------------------------------------------------------------------------------------------------------
def test_unfilled_links_and_reloads():
    pay, pats, want = text_payloads(100, 2, seed=5)
    with matchers([b"<R0>"], pats) as (dst, src):
        arena = HostArena.from_payloads(pay)
        dst.load_arena(arena)
        src.load_arena(arena)
        dst.set_meta(np.zeros(len(pay), dtype=META_DTYPE))
        dst.set_links(2)
        dst.set_rules([([dst.link(1)], []), ([0], [])])
        with raises(ESTATE, "link 1"):
            dst.scan_rules()
        dst.link_rows(0, src, "patterns", rows=0)       # the link no rule names
        dst.build_flows()
        dst.set_flowbits([(0, "set", 0)])
        for call in (dst.scan_rules, lambda: dst.scan_alerts("rules"), lambda: dst.scan_flows("rules", "flow"),
                     lambda: dst.scan_flows("rules", "packet"), dst.scan_flowbits):
            with raises(ESTATE, "link 1"):
                call()
        dst.link_rows(1, src, "patterns", rows=1)
        assert np.array_equal(dst.scan_rules(hits=True)["hits"], np.stack([want[1], want[0]]))
        # a new arena: every link is unfilled again, whatever the new arena holds
        dst.load_arena(arena)
        with raises(ESTATE, "link 1"):
            dst.scan_rules()
        check_links(dst, np.zeros((2, len(pay)), bool))
        dst.link_rows(1, src, "patterns", rows=1)
        check_links(dst, np.stack([np.zeros(len(pay), bool), want[1]]))      # link 0 of the arena before has not come back
        # rules that name no link run without one filled
        dst.load_arena(arena)
        dst.set_rules([([0], [])])
        assert np.array_equal(dst.scan_rules(hits=True)["hits"][0], want[0])


def test_set_links_zero_is_a_context_without_links():
    pay, pats, want = text_payloads(300, 3, seed=9)
    outs = []
    with matchers(pats, pats, pats) as (plain, linked, src):
        arena = HostArena.from_payloads(pay)
        for m in (plain, linked, src):
            m.load_arena(arena)
        linked.set_links(5)
        linked.link_rows(0, src, "patterns")
        linked.set_rules([([linked.link(0)], [1])])
        linked.scan_rules()
        linked.set_links(0)
        with raises(ESTATE, "no links set"):
            linked.scan_links()
        for m in (plain, linked):
            m.set_rules([([0, 1], []), ([2], [0])])
            n, W = len(pay), (len(pay) + 63) // 64
            bufs = [np.full(2, ONES, np.uint64), np.full(W, ONES, np.uint64), np.full((2, W), ONES, np.uint64), np.full(3, ONES, np.uint64)]
            _lib.gpu_check(m._g.kmpgpu_scan_rules(m._ctx, *[b.ctypes.data for b in bufs], None), "kmpgpu_scan_rules")
            outs.append(b"".join(b.tobytes() for b in bufs))
    assert outs[0] == outs[1]


def test_refusals():
    pay, pats, want = text_payloads(70, 2, seed=3)
    with matchers([b"unused"], pats, [b"unused"]) as (dst, src, other):
        arena = HostArena.from_payloads(pay)
        with raises(EINVAL, "of dst's 0 links"):
            dst.link_rows(0, src, "patterns")
        assert raw_link(dst, 0, src, 0, 0, 0, LINK_SAME, None, 0) == ESTATE                 # no links set
        dst.set_links(2)
        with raises(ESTATE, "dst has no arena"):
            dst.link_rows(0, src, "patterns")
        dst.load_arena(arena)
        src.load_arena(arena)
        other.load_arena(HostArena.from_payloads(pay[:69]))
        idx = np.zeros(70, dtype=np.uint32)
        assert raw_link(dst, 0, dst, 0, 0, 1, LINK_SAME, None, 0) == EINVAL                 # dst == src
        assert raw_link(dst, 0, None, 0, 0, 1, LINK_SAME, None, 0) == EINVAL
        assert raw_link(dst, 0, src, -1, 0, 1, LINK_SAME, None, 0) == EINVAL                # two families out of range
        assert raw_link(dst, 0, src, 4, 0, 1, LINK_SAME, None, 0) == EINVAL
        assert raw_link(dst, 0, src, 0, 0, 1, 3, idx.ctypes.data, 0) == EINVAL              # a bad map kind
        assert raw_link(dst, 0, src, 0, 0, 1, LINK_INDEX, None, 0) == EINVAL                # a NULL map where one is read
        assert raw_link(dst, 0, src, 0, 0, 1, LINK_INDEX, idx.ctypes.data, 2) == EINVAL     # map_on_device
        assert raw_link(dst, 0, src, 0, 1, 2, LINK_SAME, None, 0) == EINVAL                 # rows 1 .. 3 of 2
        assert raw_link(dst, 1, src, 0, 0, 2, LINK_SAME, None, 0) == EINVAL                 # links 1 .. 3 of 2
        assert raw_link(dst, 0, other, 0, 0, 1, LINK_SAME, None, 0) == EINVAL               # 69 payloads against 70
        with raises(ESTATE, "no rules set"):
            dst.link_rows(0, src, "rules")
        with raises(ESTATE, "no relations set"):
            dst.link_rows(0, src, "relations")
        check_links(dst, np.zeros((2, 70), bool))
        with raises(EINVAL, "link"):
            dst.set_rules([([dst.n_links + len(dst.patterns)], [])])                       # one row behind the last link
        # a source without payloads fills zeros
        dst.link_rows(0, src, "patterns")
        src.load_arena(np.zeros(0, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint32))
        dst.link_rows(0, src, "patterns", rows=0, map=np.full(70, LINK_NONE, dtype=np.uint32))
        check_links(dst, np.stack([np.zeros(70, bool), want[1]]))
