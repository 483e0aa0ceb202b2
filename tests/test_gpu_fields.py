"""kmpgpu_http_locate / kmpgpu_load_fields (GpuMatcher.http_locate, .http_spans, .load_fields) on a real MI355X: the HTTP message at the
start of every payload located on the device, and one of its fields as a packed arena that a second context owns, compared with
tests/http_model.py exactly -- span records, arena bytes including the zero padding, offsets, lengths, the present bitmap with the bits
at n and above 0, the stats, the index and the launches.

Where the kernels of csrc/kmp_fields.hip take another path:
  '\\n', "\\r\\n", ' ' and both blank-line forms at and across bytes 15|16 (two lanes) and 1023|1024 (two steps)      test_locate_boundaries
  bl == e, no '\\n' at all, L in {0, 1, 4, 5, 16, 17}, methods of 15 / 16 letters, "HTTP/" alone, 0x00 in headers   test_locate_boundaries
  64 payloads and a rest; a wavefront of 64 NONE payloads next to one with a single candidate                       test_locate_boundaries
  a '\\n' / "\\n\\r" at the payload's end with the completing '\\n' in dirty padding behind L                          test_blank_line_not_completed_behind_the_end
  every field start offset mod 16, field lengths {0, 1, 15, 16, 17, 1023, 1024, 1025}, both modes, every field      test_gather_offsets_and_lengths
  a field that ends at the payload's end in the arena's last slot, arena_bytes tight                                test_arena_tight_at_the_last_slot
  sources: borrowed with dirty padding, in place, selected, decoded, across byte 2^32                               test_sources_*
Past the grid caps: tests/test_gpu_fields_scale.py.  The command lines: tests/test_fields_cli.py.

No test provokes a fault: every negative case is one the library refuses on the host before it launches anything.

Run on a real MI355X:  python -m pytest tests/test_gpu_fields.py -m gpu
"""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import DATA

pytestmark = pytest.mark.gpu

from gpu_support import (attach_placed, attach_slots, big_buffer, check_fold, check_packets, check_rules, meta_of_flows,  # noqa: E402,F401
                         placed_base, reset, zero_slots)

import torch  # noqa: E402

import decode_model as DM  # noqa: E402
import flow_model as FM  # noqa: E402
import http_model as HM  # noqa: E402
import match_model as MM  # noqa: E402
import multithreading_string_matching_amd as K  # noqa: E402
from multithreading_string_matching_amd import _lib  # noqa: E402
from multithreading_string_matching_amd.matcher import (  # noqa: E402
    FIELD_BODY, FIELD_HEADERS, FIELD_METHOD, FIELD_NAMES, FIELD_RAW_URI, FIELD_STATUS, FIELDS_ONLY_PRESENT, HTTP_SPAN_DTYPE, OPT_NONTEMPORAL,
    OPT_REPACK, OPT_WHOLE_PAYLOAD, GpuMatcher, device_count)

EINVAL, ESTATE = -2, -3
ONES = 0xFFFFFFFFFFFFFFFF
LAUNCHES = 5                      # kmpgpu.h: field lengths, two scan kernels, index, gather
LAUNCHES_EMPTY = 3                # ... and where dst ends up without a payload; one more where the locate ran
EMPTY = (np.zeros(0, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint32))
FIELDS = list(HM.FIELDS)


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


def check_spans(m, payloads, fresh=True):
    """http_locate and the records it keeps against the model; fresh: the spans are stale, so the kernel runs"""
    stats = m.http_locate()
    assert m.last_timing().launches == (1 if fresh and payloads else 0)
    assert stats == HM.locate_stats(payloads)
    got, want = m.http_spans(), HM.spans(payloads)
    assert got.dtype == HTTP_SPAN_DTYPE == HM.SPAN_DTYPE
    if got.tobytes() != want.tobytes():
        k = next(i for i in range(len(payloads)) if got[i].tobytes() != want[i].tobytes())
        raise AssertionError(f"payload {k} ({payloads[k][:60]!r}, length {len(payloads[k])}): {got[k]}, not {want[k]}")


def fields_and_check(dst, src, payloads, field, only_present=False, located=False):
    """located: this call has to make the spans first"""
    want = HM.load_fields(payloads, field, only_present)
    res = dst.load_fields(src, field=field, only_present=only_present)
    assert first_diff(res["present"], want["present"]) is None, (field, first_diff(res["present"], want["present"]))
    assert np.array_equal(res["index"], want["index"]) and res["index"].dtype == np.int64
    assert res["stats"] == want["stats"]
    check_arena(dst, want)
    t = dst.last_timing()
    assert t.launches == (LAUNCHES if want["payloads"] else LAUNCHES_EMPTY) + (1 if located else 0) and t.kernel_ms > 0
    return want


def every_field(dst, src, payloads, fresh=True):
    """all five fields in both modes; the first call pays the locate, the ring after it does not"""
    for i, (field, only) in enumerate((f, o) for f in FIELDS for o in (False, True)):
        fields_and_check(dst, src, payloads, field, only, located=fresh and i == 0)


def filler(L, salt=0):
    """bytes without ' ', '\\r' and '\\n'"""
    base = b"0a9Fx+g/Bc7%"
    return bytes(base[(i + salt) % len(base)] for i in range(L))


# ------------------------------------------------------------------------------------------------
# 1. the locate
# ------------------------------------------------------------------------------------------------
TERMS = (b"\n", b"\r\n", b"\n\n", b"\r\n\r\n", b"\n\r\n", b"\r\n\n", b"\r", b"\n\r", b" x\n\n", b" \n\n", b" ")
PLACES = (12, 13, 14, 15, 16, 17, 1020, 1021, 1022, 1023, 1024, 1025, 2046, 2047, 2048)


def boundary_payloads():
    out = [b"dns %d" % k for k in range(64)]                       # a wavefront whose 64 payloads are all NONE ...
    out += [b"\x00\x01 binary %d" % k for k in range(64)]           # ... next to one with a single candidate
    out[100] = b"GET /only HTTP/1.1\r\nHost: a\r\n\r\nx"
    for at in PLACES:
        for term in TERMS:
            for lead in (b"GET /", b"HTTP/1.1 ", b"GET "):
                head = lead + filler(at - len(lead), at)
                out.append(head + term)
                out.append(head + term + b"H: " + filler(700, at) + b"\r\nI: " + filler(400) + term + b"tail\n\nmore")
    out += [b"GET /a\n\nB", b"GET /a\r\n\r\nB", b"HTTP/1.1 200 OK\n\n", b"GET /a HTTP/1.1", b"GET /" + filler(3000)]          # bl == e; no '\n' at all
    out += [b"", b"G", b"GET ", b"G x\n", b"HTTP", b"HTTP/", b"HTTP/\n", b"GET /0123456789a", b"GET /0123456789ab", b"HTTP/1.1 200 OK\r\n",
            b"A b\n\n" + b"1" * 11, b"A b\n\n" + b"1" * 12]                                                                       # L in {0, 1, 4, 5, 16, 17}
    out += [b"ABCDEFGHIJKLMNO /x HTTP/1.1\r\n\r\n", b"ABCDEFGHIJKLMNOP /x HTTP/1.1\r\n\r\n", b"get /x HTTP/1.1\r\n\r\n", b"GeT /x\n\n"]
    out += [b"GET /z HTTP/1.1\r\nA: \x00\x00b\r\nB: \x00\r\n\r\nbody\x00more", b"HTTP/1.1 200 \x00K\n\x00\n\n\x00"]            # 0x00 does not stop the locate
    out += [b"POST /p HTTP/1.1\r\nHost: h%d\r\n\r\nk=v" % k for k in range(70)]                                                # 64 payloads and a rest
    return out


@pytest.fixture(scope="module")
def boundaries():
    return boundary_payloads()


def test_locate_boundaries(src, dst, boundaries):
    kinds = HM.spans(boundaries)["kind"]
    assert not kinds[:64].any() and kinds[64:128].tolist().count(HM.REQUEST) == 1 and len(boundaries) % 64
    assert {int(k) for k in kinds} == {HM.NONE, HM.REQUEST, HM.RESPONSE}
    try:
        reset(src, dst)
        src.load_arena(K.HostArena.from_payloads(boundaries))
        check_spans(src, boundaries)
        check_spans(src, boundaries, fresh=False)                   # valid spans: nothing is launched, the same answers
        every_field(dst, src, boundaries, fresh=False)
    finally:
        reset(src, dst)


def test_blank_line_not_completed_behind_the_end(src, dst):
    """a '\\n' as the last byte and "\\n\\r" as the last two bytes, each with the completing '\\n' in dirty padding behind L -- in the same
    lane, the next lane, the next step -- and at a slot's end with the next slot beginning with it"""
    payloads = []
    for L in (23, 30, 31, 33, 1022, 1023, 1025, 1026, 2047):
        for head in (b"GET /a\r\nH: ", b"HTTP/1.1 200 OK\r\nS: "):
            for end in (b"\n", b"\n\r"):
                payloads.append(head + filler(L - len(head) - len(end), L) + end)
    for L in (16, 1024):                                                    # whole slots: the next slot holds what would complete it
        payloads += [b"GET /a\r\nH: " + filler(L - 12, L) + b"\n", b"\nrest", b"GET /a\r\nH: " + filler(L - 13, L) + b"\n\r", b"\n\nrest"]
    slots = [t + b"\n" * ((-len(t)) % 16) for t in payloads]
    padded = [s for s, t in zip(slots, payloads) if len(s) > len(t)]
    assert len(padded) >= 36 and all(HM.locate(s)["bl"] is not None for s in padded if not s.startswith(b"\n"))      # the padding would complete them
    want = HM.spans(payloads)
    assert not (want["flags"] & HM.HAS_BLANK).any() and (want["kind"] != HM.NONE).sum() == 40
    try:
        reset(src, dst)
        keep = attach_slots(src, payloads, slots)
        check_spans(src, payloads)
        every_field(dst, src, payloads, fresh=False)
        del keep
    finally:
        reset(src, dst)
        src.load_arena(*EMPTY)


# ------------------------------------------------------------------------------------------------
# 2. the gather
# ------------------------------------------------------------------------------------------------
LENGTHS = (0, 1, 15, 16, 17, 1023, 1024, 1025)


def gather_payloads():
    out = []
    for i, F in enumerate(LENGTHS):
        for s in range(16):
            # RAW_URI of length F behind a method of 1 .. 15 letters (start offsets 2 .. 16)
            if s:
                out.append(b"ABCDEFGHIJKLMNO"[:s] + b" " + filler(F, s) + b" HTTP/1.1\r\nH: " + filler(s + i) + b"\r\n\r\n" + filler(3 * s))
            # HEADERS of length F at start offset 6 + s: bl == e for F == 0, otherwise F - 1 bytes and their '\n' (a single '\n' would be
            # the blank line itself); and headers that the segment cut, to the payload's end
            line = b"GET /" + filler(s, i)
            if F != 1:
                out.append(line + b"\n" + (filler(F - 1, s) + b"\n" if F else b"") + b"\n" + filler(s))
            out.append(line + b"\n" + filler(F, s))
            # BODY of length F at start offset 9 + s and 10 + s (the two blank-line forms), to the payload's end
            out.append(line + b"\nH\n\n" + filler(F, s))
            out.append(line + b"\nH\n\r\n" + filler(F, s))
            # STATUS of length F
            out.append(b"HTTP/1." + filler(s) + b" " + filler(F, i) + b" OK\r\n\r\n")
    return out


@pytest.mark.parametrize("nontemporal", [1, 0])
def test_gather_offsets_and_lengths(src, dst, nontemporal):
    payloads = gather_payloads()
    seen = {f: set() for f in FIELDS}
    for t in payloads:
        r = HM.locate(t)
        for f in FIELDS:
            if r[f] is not None:
                seen[f].add((r[f][0] % 16, r[f][1]))
    for f in ("headers", "body"):
        assert {(o, F) for o in range(16) for F in LENGTHS} <= seen[f]                  # every start offset mod 16 x every length
    assert {(o % 16, F) for o in range(2, 17) for F in LENGTHS} <= seen["raw_uri"] and {(0, F) for F in range(1, 16)} <= seen["method"]
    try:
        reset(src, dst)
        dst.set_option(OPT_NONTEMPORAL, nontemporal)
        src.load_arena(K.HostArena.from_payloads(payloads))
        every_field(dst, src, payloads)
    finally:
        reset(src, dst)


def test_arena_tight_at_the_last_slot(src, dst):
    """the body, and headers that the segment cut, end at the payload's end; the last payload fills its slot and the arena ends there"""
    for head in (b"GET /tight HTTP/1.1\r\nHost: abc\r\n\r\n", b"GET /tight HTTP/1.1\r\nHost: "):
        last = head + filler(48 - len(head))
        payloads = [b"HTTP/1.1 200 OK\r\n\r\n" + filler(13), b"x" * 31, b"", last]
        slots = zero_slots(payloads)
        assert len(slots[-1]) == len(payloads[-1]) == 48                                  # no padding behind the last payload
        ln = np.array([len(t) for t in payloads], dtype=np.int32)
        size = np.array([len(s) for s in slots], dtype=np.int64)
        d = (torch.from_numpy(np.frombuffer(b"".join(slots), dtype=np.uint8).copy()).cuda(), torch.from_numpy(np.cumsum(size) - size).cuda(),
             torch.from_numpy(ln).cuda())
        torch.cuda.synchronize()
        try:
            reset(src, dst)
            src.attach_arena(*d, arena_bytes=int(size.sum()))
            check_spans(src, payloads)
            every_field(dst, src, payloads, fresh=False)
        finally:
            reset(src, dst)
            src.load_arena(*EMPTY)


# ------------------------------------------------------------------------------------------------
# 3. every kind of source
# ------------------------------------------------------------------------------------------------
def traffic(n, seed):
    """requests, responses, cut messages and other traffic, lengths 0 .. 2500"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        kind = int(rng.integers(0, 6))
        nl = b"\r\n" if rng.random() < 0.7 else b"\n"
        hdrs = b"".join(b"H%d: " % i + filler(int(rng.integers(0, 300)), k + i) + nl for i in range(int(rng.integers(0, 5))))
        body = filler(int(rng.integers(0, 1200)), k)
        if kind <= 1:
            t = (b"GET", b"POST", b"OPTIONS", b"X")[k % 4] + b" /" + filler(int(rng.integers(0, 200)), k) + b" HTTP/1.1" + nl + hdrs + nl + body
        elif kind == 2:
            t = b"HTTP/1.1 %d OK" % (200 + k % 300) + nl + hdrs + nl + body
        elif kind == 3:
            t = (b"PUT /cut " + filler(20) + nl + hdrs + body)[:int(rng.integers(0, 400))]
        else:
            t = rng.integers(0, 256, int(rng.integers(0, 200)), dtype=np.uint8).tobytes()
        out.append(t)
    return out


def test_sources_borrowed_with_dirty_padding(src, dst):
    payloads = traffic(400, seed=61)
    slots = [t + (b"\r\n\r\n GET" * 4)[:(-len(t)) % 16 or (0 if t else 16)] for t in payloads]
    assert sum(len(s) > len(t) for s, t in zip(slots, payloads)) > 300
    try:
        reset(src, dst)
        keep = attach_slots(src, payloads, slots)
        before = keep[0].cpu().numpy().copy()
        check_spans(src, payloads)
        every_field(dst, src, payloads, fresh=False)
        assert np.array_equal(keep[0].cpu().numpy(), before)
    finally:
        reset(src, dst)
        src.load_arena(*EMPTY)


@pytest.mark.parametrize("repack", [0, 1])
def test_sources_with_gaps_and_shuffled_slots(src, dst, repack):
    rng = np.random.default_rng(62)
    payloads = traffic(300, seed=62)
    ln = np.array([len(t) for t in payloads], dtype=np.int64)
    slot = np.maximum(16, (ln + 15) & ~15)
    order = rng.permutation(len(payloads))
    adv = 16 * rng.integers(0, 4, len(payloads)) + slot[order]
    off = np.zeros(len(payloads), dtype=np.int64)
    off[order] = np.cumsum(adv) - slot[order]
    arena = np.frombuffer((b"\n\r\n" * (int(adv.sum()) // 3 + 40))[:int(adv.sum()) + 64], dtype=np.uint8).copy()      # gaps and padding: blank lines
    for o, t in zip(off, payloads):
        arena[int(o):int(o) + len(t)] = np.frombuffer(t, dtype=np.uint8)
    try:
        reset(src, dst)
        src.set_option(OPT_REPACK, repack)
        src.load_arena(arena, off.astype(np.uint64), ln.astype(np.uint32))
        if not repack:
            assert first_diff(src.arena_download()[1], off) is None            # not packed: the index is followed as it is
        every_field(dst, src, payloads)
    finally:
        reset(src, dst)


def test_sources_selected_and_decoded(src, dst, third):
    payloads = traffic(300, seed=63) + [b"GET /%61dmin%20x HTTP/1.1\r\nA: %0d%0a%0d%0a\r\n\r\n%0A%0Abody", b"GET%20/x HTTP/1.1\n\n"]
    pick = np.arange(len(payloads)) % 3 != 1
    try:
        reset(src, dst, third)
        src.load_arena(K.HostArena.from_payloads(payloads))
        third.load_selected(src, pick)
        every_field(dst, third, [t for t, p in zip(payloads, pick) if p])
        third.load_decoded(src)
        decoded = [DM.decode(t) for t in payloads]
        assert HM.locate(decoded[-2])["raw_uri"] == (4, 6) and HM.locate(decoded[-1])["kind"] == HM.REQUEST        # the escapes make structure
        every_field(dst, third, decoded)
        # a field buffer is a source like any other: the request line inside a body, and back into the first context
        bodies = fields_and_check(third, src, payloads, "body", located=True)["payloads"]
        every_field(dst, third, bodies)
    finally:
        reset(src, dst, third)


def test_high_offsets(src, dst, big_buffer):
    """source offsets in front of, across and behind 2^32: payload k straddles it, its wavefront has lanes on both sides"""
    payloads = traffic(200, seed=64)
    k = 70
    payloads[k] = b"POST /" + filler(30) + b" HTTP/1.1\r\nA: " + filler(20) + b"\r\nB: " + filler(1100, 1) + b"\r\n\r\n" + filler(900, 2)
    payloads[k - 1] = b"GET /" + filler(24) + b"\r\n\r"
    try:
        reset(src, dst)
        keep = attach_placed(src, payloads, None, placed_base("split", payloads, k=k), big_buffer)
        check_spans(src, payloads)
        every_field(dst, src, payloads, fresh=False)
        del keep
    finally:
        reset(src, dst)
        src.load_arena(*EMPTY)


# ------------------------------------------------------------------------------------------------
# 4. composition
# ------------------------------------------------------------------------------------------------
def test_the_rule_the_feature_is_for(src, dst, third):
    """`/admin` in the request line, escaped or not, against `/admin` in a Referer: header, in a request body and in a response body"""
    pats = [b"/admin"]
    rules = [([0], [])]
    payloads = [b"GET /%61dmin HTTP/1.1\r\nHost: intranet\r\n\r\n",
                b"GET /index.html HTTP/1.1\r\nReferer: http://intranet/admin\r\n\r\n",
                b"POST /login HTTP/1.1\r\nHost: intranet\r\n\r\nnext=/admin&password=x",
                b"HTTP/1.1 200 OK\r\n\r\n<a href=/admin>",
                b"GET /admin/users HTTP/1.1\r\n\r\n",
                b"not http at all /admin"]
    try:
        reset(src, dst, third)
        for m in (src, dst, third):
            m.set_patterns(pats); m.set_rules(rules)
        src.load_arena(K.HostArena.from_payloads(payloads))
        uris = fields_and_check(dst, src, payloads, "raw_uri", located=True)["payloads"]
        assert uris == [b"/%61dmin", b"/index.html", b"/login", b"", b"/admin/users", b""]
        want = DM.load_decoded(uris)
        res = third.load_decoded(dst)
        assert res["stats"] == want["stats"] and want["payloads"][0] == b"/admin"
        check_arena(third, want)
        for m, texts, fires in ((src, payloads, [False, True, True, True, True, True]), (dst, uris, [False, False, False, False, True, False]),
                                (third, want["payloads"], [True, False, False, False, True, False])):
            st = MM.starts(texts, pats)
            res = check_rules(m, MM.hits(st), rules, MM.counts(st))
            assert res["hits"][0].tolist() == fires
        # the spans survive the scan, and so does the rest of src
        check_spans(src, payloads, fresh=False)
    finally:
        reset(src, dst, third)
        for m in (src, dst, third):
            m.set_patterns([b"x"])


def test_flows_metadata_and_the_device_bitmap(src, dst, third):
    payloads = traffic(300, seed=65)
    n = len(payloads)
    meta = meta_of_flows(np.arange(n) // 4 % 23)
    g = _lib.gpu_lib()
    try:
        reset(src, dst, third)
        src.load_arena(K.HostArena.from_payloads(payloads))
        src.set_meta(meta)
        src.build_flows()
        ids = src.flow_ids()
        want = fields_and_check(dst, src, payloads, "raw_uri", located=True)
        assert dst.meta().tobytes() == meta.tobytes()
        dst.build_flows()
        assert np.array_equal(dst.flow_ids(), ids) and np.array_equal(ids, FM.flow_of_np(meta))          # the capture's flow numbers
        want = fields_and_check(dst, src, payloads, "status", only_present=True)
        assert 0 < len(want["index"]) < n and dst.meta().tobytes() == meta[want["index"]].tobytes()       # ... and the present ones' records
        # the device bitmap, handed to kmpgpu_load_selected of a third context: the raw payloads of the same set
        W = (n + 63) // 64
        words = np.full(W, np.uint64(ONES))
        d_present = C.c_void_p()
        st = _lib.FieldsStats()
        assert g.kmpgpu_load_fields(dst._ctx, src._ctx, FIELD_BODY, FIELDS_ONLY_PRESENT, words.ctypes.data, C.byref(d_present), C.byref(st)) == 0
        have = HM.load_fields(payloads, "body", True)
        assert np.array_equal(words, have["words"])                                                      # the bits at n and above are 0
        assert d_present.value and st.n_payloads == st.n_present == len(have["index"])
        n_sel = C.c_uint64()
        assert g.kmpgpu_load_selected(third._ctx, src._ctx, d_present, 1, C.byref(n_sel)) == 0 and n_sel.value == st.n_present
        check_arena(third, dict(zip(("arena", "off", "len"), DM.packed_image([payloads[int(k)] for k in have["index"]]))))
    finally:
        reset(src, dst, third)


def test_spans_life_cycle(src, dst):
    """dropped by every loader, made again by the next load_fields; read in ranges; refused where there are none"""
    g = _lib.gpu_lib()
    a, b = traffic(150, seed=66), traffic(90, seed=67)
    out = np.zeros(4, dtype=HTTP_SPAN_DTYPE)
    try:
        reset(src, dst)
        src.set_patterns([b"GET"])
        src.load_arena(K.HostArena.from_payloads(a))
        assert g.kmpgpu_http_spans_read(src._ctx, out.ctypes.data, 0, 1) == ESTATE and b"no spans" in g.kmpgpu_last_error()
        fields_and_check(dst, src, a, "headers", located=True)
        assert src.http_spans().tobytes() == HM.spans(a).tobytes()
        assert g.kmpgpu_http_spans_read(src._ctx, out.ctypes.data, 146, 4) == 0 and out.tobytes() == HM.spans(a[146:]).tobytes()
        assert g.kmpgpu_http_spans_read(src._ctx, out.ctypes.data, 147, 4) == EINVAL and g.kmpgpu_http_spans_read(src._ctx, None, 0, 1) == EINVAL
        assert g.kmpgpu_http_spans_read(None, out.ctypes.data, 0, 1) == EINVAL and g.kmpgpu_http_locate(None, None) == EINVAL
        src.scan()
        fields_and_check(dst, src, a, "body")                                     # a scan keeps them
        src.load_arena(K.HostArena.from_payloads(b))                              # a loader drops them
        assert g.kmpgpu_http_spans_read(src._ctx, out.ctypes.data, 0, 1) == ESTATE
        fields_and_check(dst, src, b, "body", located=True)
        check_spans(src, b, fresh=False)
        assert g.kmpgpu_http_spans_read(dst._ctx, out.ctypes.data, 0, 1) == ESTATE             # dst's own are not src's
        src.load_arena(*EMPTY)
        assert src.http_locate() == {"n_requests": 0, "n_responses": 0, "n_blank": 0, "bytes_scanned": 0} and src.http_spans().shape == (0,)
    finally:
        reset(src, dst)


def test_src_untouched(src, dst, oracle):
    payloads = traffic(300, seed=68)
    pats = [b"HTTP/1.1", b"GET ", b"H1: ", b"\r\n\r\n"]
    try:
        reset(src, dst)
        src.set_patterns(pats)
        src.set_option(OPT_WHOLE_PAYLOAD, 1)
        src.load_arena(K.HostArena.from_payloads(payloads))
        before, arena_before = src.scan_packets(hits=True), src.arena_download()
        assert before["counts"].tolist() == list(MM.counts(MM.starts(payloads, pats, whole=True))) and any(before["counts"])
        every_field(dst, src, payloads)
        after, arena_after = src.scan_packets(hits=True), src.arena_download()
        assert all(np.array_equal(before[f], after[f]) for f in ("hits", "any", "pkt_counts", "counts"))
        assert all(np.array_equal(x, y) for x, y in zip(arena_before, arena_after))
    finally:
        reset(src, dst)
        src.set_patterns([b"x"])


# ------------------------------------------------------------------------------------------------
# 5. errors, through the raw ABI
# ------------------------------------------------------------------------------------------------
def test_errors(src, dst):
    g = _lib.gpu_lib()
    payloads = traffic(120, seed=69)
    kept = traffic(77, seed=70)
    want_kept = dict(zip(("arena", "off", "len"), DM.packed_image(kept)))
    st = _lib.FieldsStats()
    d_present = C.c_void_p()
    words = np.zeros(8, dtype=np.uint64)

    def call(d, s, field=FIELD_RAW_URI, flags=0):
        st.n_payloads = 12345
        d_present.value = 1
        return g.kmpgpu_load_fields(d, s, field, flags, words.ctypes.data, C.byref(d_present), C.byref(st))

    def dst_keeps_its_arena(rc, code, what):
        assert rc == code, (rc, code)
        msg = g.kmpgpu_last_error()
        assert b"kmpgpu_load_fields" in msg and what in msg, msg
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
        dst_keeps_its_arena(call(dst._ctx, src._ctx, field=6), EINVAL, b"field 6")
        dst_keeps_its_arena(call(dst._ctx, src._ctx, flags=2), EINVAL, b"flag bits")
        dst_keeps_its_arena(call(dst._ctx, src._ctx, flags=0x80000001), EINVAL, b"flag bits")
        with pytest.raises(ValueError):
            dst.load_fields(src, field="uri")
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
                assert g.kmpgpu_http_locate(other._ctx, None) == ESTATE and b"kmpgpu_http_locate" in g.kmpgpu_last_error()
                n_pay = C.c_uint64()
                assert g.kmpgpu_load_frames_finish(other._ctx, C.byref(n_pay)) == 0
        finally:
            _lib.host_lib().kmp_frames_free(C.byref(fr))
        # src without an arena: dst empty, nothing handed out
        src.load_arena(*EMPTY)
        assert call(dst._ctx, src._ctx, flags=FIELDS_ONLY_PRESENT) == 0
        assert dst.arena_info() == (0, 0) and st.n_payloads == 0 and not d_present.value
        res = dst.load_fields(src)
        assert res["present"].shape == (0,) and res["index"].shape == (0,) and res["stats"]["n_payloads"] == 0
        # no payload has the field: dst without an arena, three launches and the locate
        none = [b"dns", b"", b"\x00" * 40]
        src.load_arena(K.HostArena.from_payloads(none))
        fields_and_check(dst, src, none, "method", only_present=True, located=True)
        # NULL outputs
        src.load_arena(K.HostArena.from_payloads(payloads))
        assert g.kmpgpu_load_fields(dst._ctx, src._ctx, FIELD_HEADERS, 0, None, None, None) == 0
        check_arena(dst, HM.load_fields(payloads, "headers"))
        assert dst.last_timing().launches == LAUNCHES + 1
    finally:
        reset(src, dst)


def test_two_devices_are_refused(src):
    if device_count() < 2:
        pytest.skip("one device")
    g = _lib.gpu_lib()
    with GpuMatcher(1) as far:
        src.load_arena(K.HostArena.from_payloads([b"GET / HTTP/1.1\r\n\r\n", b"", b"x" * 40]))
        assert g.kmpgpu_load_fields(far._ctx, src._ctx, FIELD_METHOD, 0, None, None, None) == EINVAL
        assert b"kmpgpu_load_fields" in g.kmpgpu_last_error() and far.arena_info() == (0, 0)


def test_constants():
    assert FIELD_NAMES == HM.FIELDS and (FIELD_METHOD, FIELD_RAW_URI, FIELD_STATUS, FIELD_HEADERS, FIELD_BODY) == (1, 2, 3, 4, 5)
    assert (K.FIELD_BODY, K.FIELDS_ONLY_PRESENT) == (5, 1)
