"""kmpgpu_load_base64 (GpuMatcher.load_base64) on a real MI355X: the base64 runs of a context's payloads decoded on the device into a
packed arena that a second context owns, compared with tests/base64_model.py exactly -- arena bytes including the zero padding,
offsets, lengths, the changed bitmap with the bits at n and above 0, the stats and the index.

Where the kernels of csrc/kmp_base64.hip take another path:
  a run's start, end and min_run-th byte on either side of a unit (16), a step (1024), the unroll (4096)        test_boundaries
  every start offset mod 16 with every m % 4; '=' split across a unit's and a step's edge                       test_boundaries
  a run of min_run - 1 that ends on a step's edge (the look-ahead finds nothing), and one byte longer           test_boundaries
  the run offset mod 4 carried over many steps; payloads of 0..3 and of exactly min_run bytes                   test_sizes
  nothing behind a payload's end takes part: dirty padding, the next slot                                       test_sources_*
  a step without a decoded run at a 16-byte aligned output position (the straight copy) / any other one         test_sizes, test_only_changed[none]
  source offsets across and behind 2^32                                                                         test_high_offsets
Past the grid caps and destinations past 2^32: tests/test_gpu_base64_scale.py.

No test provokes a fault: every negative case is one the library refuses on the host before it launches anything.

Run on a real MI355X:  python -m pytest tests/test_gpu_base64.py -m gpu
"""
import base64
import ctypes as C
import os

import numpy as np
import pytest

from conftest import DATA

pytestmark = pytest.mark.gpu

from gpu_support import (attach_placed, attach_slots, big_buffer, check_fold, check_packets, check_rules, meta_of_flows,  # noqa: E402,F401
                         placed_base, reset, run_cli, strip_elapsed)

import base64_model as B6  # noqa: E402
import bytetest_model as BM  # noqa: E402
import decode_model as DM  # noqa: E402
import flow_model as FM  # noqa: E402
import match_model as MM  # noqa: E402
import multithreading_string_matching_amd as K  # noqa: E402
import regex_model as RX  # noqa: E402
from multithreading_string_matching_amd import _lib  # noqa: E402
from multithreading_string_matching_amd.matcher import B64_ONLY_CHANGED, B64_URLSAFE, OPT_NONTEMPORAL, OPT_REPACK, GpuMatcher, device_count  # noqa: E402

EINVAL, ESTATE = -2, -3
ONES = 0xFFFFFFFFFFFFFFFF
LAUNCHES = 5                      # kmpgpu.h: base64 lengths, two scan kernels, index, write
LAUNCHES_EMPTY = 3                # ... and where dst ends up without a payload
EMPTY = (np.zeros(0, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint32))
MIN_RUNS = [4, 16, 255]


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


def decode_and_check(dst, src, payloads, min_run=16, urlsafe=False, only_changed=False):
    want = B6.load_base64(payloads, min_run, urlsafe, only_changed)
    res = dst.load_base64(src, min_run=min_run, urlsafe=urlsafe, only_changed=only_changed)
    assert first_diff(res["changed"], want["changed"]) is None, first_diff(res["changed"], want["changed"])
    assert np.array_equal(res["index"], want["index"]) and res["index"].dtype == np.int64
    assert res["stats"] == want["stats"]
    check_arena(dst, want)
    t = dst.last_timing()
    assert t.launches == (LAUNCHES if want["payloads"] else LAUNCHES_EMPTY) and t.kernel_ms > 0
    return want


def payloads_of(m):
    a, off, ln = m.arena_download()
    return [a[int(o):int(o) + int(n)].tobytes() for o, n in zip(off, ln)]


def alpha(n, urlsafe=False, salt=0):
    """n alphabet bytes, the two behind the digits among them"""
    chars = (B6.URL if urlsafe else B6.STD)
    return bytes(chars[(7 * (i + salt) + (i + salt) // 9) % 64] for i in range(n))


def filler(L, urlsafe=False, salt=0):
    """bytes outside the alphabet: the other alphabet's two, blanks, '%', line ends, 0x00, 0xFF -- and no '='"""
    base = (b"+ /.:%\r\n\x00\xff" if urlsafe else b"- _.:%\r\n\x00\xff")
    return bytes(base[(i + salt) % len(base)] for i in range(L))


def with_run(L, s, m, urlsafe, tail=b"", salt=0):
    """a payload of L bytes outside the alphabet with one run [s, s + m) and `tail` directly behind it"""
    assert 0 <= s and s + m + len(tail) <= L
    b = bytearray(filler(L, urlsafe, salt))
    b[s:s + m] = alpha(m, urlsafe, salt)
    b[s + m:s + m + len(tail)] = tail
    return bytes(b)


# ------------------------------------------------------------------------------------------------
# boundaries
# ------------------------------------------------------------------------------------------------
def boundary_payloads(mr, urlsafe):
    out = []
    unit = (mr + 23) // 16 * 16                          # a unit's edge with room for a run of min_run + 3 in front of it
    for E in (16, unit, 1024, 4096):
        L = E + mr + 48
        for side in (E - 1, E):
            for m in (mr - 1, mr, mr + 1, mr + 6):
                out.append(with_run(L, side, m, urlsafe, b"==", salt=E + m))                   # the run's start
                if side + 1 - m >= 0:
                    out.append(with_run(L, side + 1 - m, m, urlsafe, b"==", salt=E + m + 1))   # its last byte
                if side - (mr - 1) >= 0:
                    out.append(with_run(L, side - (mr - 1), m, urlsafe, b"=", salt=E + m + 2))  # its min_run-th byte
            for m in (3, 5):                                                                # short runs on the edge: copied
                out.append(with_run(L, side - 2, m, urlsafe, b"==", salt=E))
    # every start offset mod 16 with every m % 4
    for s in range(16, 32):
        for j in range(4):
            out.append(with_run(s + mr + j + 24, s, mr + j, urlsafe, b"===", salt=s + j))
    # '=' split across a unit's and a step's edge: the run ends 2, 1, 0 bytes in front of the edge
    for E in (unit, 1024, 4096):
        for m in range(mr, mr + 4):
            for back in (2, 1, 0):
                out.append(with_run(E + 40, E - back - m, m, urlsafe, b"===", salt=E + m + back))
                out.append(with_run(E + 40, E - back - m, m, urlsafe, b"=", salt=E + m + back))
    # a run of min_run - 1 that ends on a step's edge, a byte outside the alphabet behind it; and the same run one byte longer
    for E in (1024, 2048, 4096):
        out.append(with_run(E + 300, E - (mr - 1), mr - 1, urlsafe, salt=E))
        out.append(with_run(E + 300, E - (mr - 1), mr, urlsafe, salt=E))
        out.append(with_run(E + 300, E - (mr - 1), mr + 253, urlsafe, b"=", salt=E))         # ... and far past the look-ahead
        out.append(with_run(E + 2, E - (mr - 1), mr + 1, urlsafe, salt=E))                    # the payload ends behind the edge
        out.append(with_run(E, E - (mr - 1), mr - 1, urlsafe, salt=E))                        # ... and on it
    return out


@pytest.mark.parametrize("only_changed", [False, True])
@pytest.mark.parametrize("urlsafe", [False, True])
@pytest.mark.parametrize("mr", MIN_RUNS)
def test_boundaries(src, dst, mr, urlsafe, only_changed):
    payloads = boundary_payloads(mr, urlsafe)
    try:
        reset(src, dst)
        src.load_arena(K.HostArena.from_payloads(payloads))
        want = decode_and_check(dst, src, payloads, mr, urlsafe, only_changed)
        assert 0 < want["stats"]["n_changed"] < len(payloads)
    finally:
        reset(src, dst)


# ------------------------------------------------------------------------------------------------
# sizes
# ------------------------------------------------------------------------------------------------
def plain(rng, L):
    """hostile bytes with a blank at every 8th place: no run of 8"""
    t = bytearray(B6.random_payload(rng, L))
    t[7::8] = b" " * len(t[7::8])
    return bytes(t)


def blob(rng, n, urlsafe=False, pad=True):
    return B6.encode(rng.integers(0, 256, n, dtype=np.uint8).tobytes(), urlsafe, pad)


def size_payloads(kind, mr, urlsafe):
    rng = np.random.default_rng({"long_run": 1, "tiny": 2, "64_bytes": 3, "hostile": 4}[kind] + mr)
    if kind == "long_run":          # the carried offset mod 4 over 20 steps, from every offset mod 4, with every padding
        return [filler(s, urlsafe) + alpha(20000 + j, urlsafe, s) + b"=" * e + filler(5, urlsafe) for s in range(4) for j in (0, 2, 3) for e in (0, 2)]
    if kind == "tiny":
        out = [b"", b"Q", b"QU", b"QUJ", b"=", b"==", alpha(mr, urlsafe), alpha(mr - 1, urlsafe), alpha(mr, urlsafe)[:-1] + b".",
               b"." + alpha(mr, urlsafe), alpha(mr + 1, urlsafe), alpha(mr + 2, urlsafe) + b"==", b"", alpha(mr + 3, urlsafe) + b"="]
        return out * 6              # more than one wavefront's group of 64
    if kind == "64_bytes":          # two runs of 64 payloads and a rest, several runs each
        out = []
        for k in range(130):
            t = b""
            while len(t) < 64:
                t += blob(rng, int(rng.integers(1, 14)), urlsafe, pad=bool(k & 1)) + filler(int(rng.integers(1, 4)), urlsafe, k)
            out.append(t[:64])
        out[5], out[64], out[129] = filler(64, urlsafe), alpha(64, urlsafe), filler(60, urlsafe) + alpha(4, urlsafe)
        return out
    return [B6.random_payload(rng, int(L)) for L in rng.integers(0, 3001, 150)]


@pytest.mark.parametrize("urlsafe", [False, True])
@pytest.mark.parametrize("kind, mr", [("long_run", 16), ("long_run", 255), ("tiny", 4), ("tiny", 16), ("tiny", 255), ("64_bytes", 4), ("64_bytes", 16),
                                      ("hostile", 4), ("hostile", 5)])
def test_sizes(src, dst, kind, mr, urlsafe):
    payloads = size_payloads(kind, mr, urlsafe)
    try:
        reset(src, dst)
        src.load_arena(K.HostArena.from_payloads(payloads))
        for only_changed in (False, True):
            decode_and_check(dst, src, payloads, mr, urlsafe, only_changed)
        # the other instantiation of the write kernel
        dst.set_option(OPT_NONTEMPORAL, 0)
        decode_and_check(dst, src, payloads, mr, urlsafe, False)
    finally:
        reset(src, dst)


def test_nothing_to_decode_is_a_copy(src, dst, third):
    """no run of min_run: byte for byte what kmpgpu_load_selected with all bits set makes of the source"""
    rng = np.random.default_rng(5)
    payloads = [plain(rng, int(L)) for L in rng.integers(0, 3001, 200)]
    try:
        reset(src, dst, third)
        src.load_arena(K.HostArena.from_payloads(payloads))
        want = decode_and_check(dst, src, payloads, 8)
        assert want["stats"]["n_changed"] == 0 and want["payloads"] == payloads
        third.load_selected(src, np.ones(len(payloads), dtype=bool))
        assert all(np.array_equal(x, y) for x, y in zip(dst.arena_download(), third.arena_download()))
        decode_and_check(dst, src, payloads, 8, only_changed=True)
        assert dst.arena_info() == (0, 0)
    finally:
        reset(src, dst, third)


# ------------------------------------------------------------------------------------------------
# KMPGPU_B64_ONLY_CHANGED, the device bitmap, the metadata
# ------------------------------------------------------------------------------------------------
def mix(n, which, urlsafe=False):
    rng = np.random.default_rng(n)
    out = []
    for k in range(n):
        t = plain(rng, int(rng.integers(0, 200)))
        if which(k):
            t = t[:len(t) // 2] + b" " + blob(rng, 12 + k % 7, urlsafe) + b" " + t[len(t) // 2:]
        out.append(t)
    return out


@pytest.mark.parametrize("name", ["every_third", "none", "all", "word_boundary"])
def test_only_changed(src, dst, third, name):
    n, which = {"every_third": (300, lambda k: k % 3 == 1), "none": (300, lambda k: False), "all": (300, lambda k: True),
                "word_boundary": (129, lambda k: k in (63, 64, 128))}[name]
    payloads = mix(n, which)
    meta = meta_of_flows(np.arange(n) // 4 % 23)
    g = _lib.gpu_lib()
    try:
        reset(src, dst, third)
        src.load_arena(K.HostArena.from_payloads(payloads))
        src.set_meta(meta)
        for only in (True, False):
            want = decode_and_check(dst, src, payloads, 16, False, only)
            assert want["changed"].tolist() == [which(k) for k in range(n)]
            if len(want["index"]):
                assert dst.meta().tobytes() == meta[want["index"]].tobytes()          # the metadata follows in both modes
            else:
                assert dst.arena_info() == (0, 0)
        # the device bitmap, handed to kmpgpu_load_selected of a third context: the raw payloads of the same set
        W = (n + 63) // 64
        words = np.full(W, np.uint64(ONES))
        d_changed = C.c_void_p()
        st = _lib.DecodeStats()
        assert g.kmpgpu_load_base64(dst._ctx, src._ctx, 16, B64_ONLY_CHANGED, words.ctypes.data, C.byref(d_changed), C.byref(st)) == 0
        assert np.array_equal(words, B6.words([which(k) for k in range(n)]))         # the bits at n and above are 0
        assert d_changed.value and st.n_payloads == st.n_changed == sum(which(k) for k in range(n))
        n_sel = C.c_uint64()
        assert g.kmpgpu_load_selected(third._ctx, src._ctx, d_changed, 1, C.byref(n_sel)) == 0 and n_sel.value == st.n_changed
        raw = [payloads[k] for k in range(n) if which(k)]
        check_arena(third, dict(zip(("arena", "off", "len"), B6.packed_image(raw))))
    finally:
        reset(src, dst, third)


# ------------------------------------------------------------------------------------------------
# every kind of source
# ------------------------------------------------------------------------------------------------
def tail_payloads(n, seed, mr):
    """every payload ends inside a run: of min_run - 1 (a byte more would decode it), of min_run + 2 or + 3 (a '=' more would be
    dropped), or of a few bytes"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        L = int(rng.choice([0, 1, 2, 14, 15, 16, 17, 30, 31, 32, 100, 1023, 1024, 1500]))
        m = min(L, (mr - 1, mr + 2, mr + 3, 3)[k % 4])
        head = plain(rng, L - m)
        out.append(head[:-1] + b"."[:len(head)] + alpha(m, salt=k))                   # (the run is these m bytes and no more)
    return out


def test_sources_borrowed_with_dirty_padding(src, dst):
    """the padding holds alphabet bytes and '=': nothing behind a payload's end makes its last run longer or pads it"""
    mr = 8
    payloads = tail_payloads(600, seed=31, mr=mr)
    slots = [t + ((b"QUJD" if k & 1 else b"==QU") * 4)[:(-len(t)) % 16 or (0 if t else 16)] for k, t in enumerate(payloads)]
    assert sum(len(s) > len(t) for s, t in zip(slots, payloads)) > 400
    assert sum(B6.changed(s, mr) and not B6.changed(t, mr) for s, t in zip(slots, payloads)) > 50     # the padding would decode them
    try:
        reset(src, dst)
        keep = attach_slots(src, payloads, slots)
        before = keep[0].cpu().numpy().copy()
        for urlsafe, only_changed in ((False, False), (True, False), (False, True)):
            decode_and_check(dst, src, payloads, mr, urlsafe, only_changed)
        assert np.array_equal(keep[0].cpu().numpy(), before)
    finally:
        reset(src, dst)
        src.load_arena(*EMPTY)


@pytest.mark.parametrize("repack", [0, 1])
def test_sources_with_gaps_and_shuffled_slots(src, dst, repack):
    rng = np.random.default_rng(32)
    mr = 8
    payloads = tail_payloads(500, seed=32, mr=mr)
    ln = np.array([len(t) for t in payloads], dtype=np.int64)
    slot = np.maximum(16, (ln + 15) & ~15)
    order = rng.permutation(len(payloads))
    adv = 16 * rng.integers(0, 4, len(payloads)) + slot[order]
    off = np.zeros(len(payloads), dtype=np.int64)
    off[order] = np.cumsum(adv) - slot[order]
    arena = np.frombuffer((b"QUJDRA==" * (int(adv.sum()) // 8 + 40))[:int(adv.sum()) + 64], dtype=np.uint8).copy()      # gaps and padding: base64
    for o, t in zip(off, payloads):
        arena[int(o):int(o) + len(t)] = np.frombuffer(t, dtype=np.uint8)
    try:
        reset(src, dst)
        src.set_option(OPT_REPACK, repack)
        src.load_arena(arena, off.astype(np.uint64), ln.astype(np.uint32))
        if not repack:
            assert first_diff(src.arena_download()[1], off) is None            # not packed: the index is followed as it is
        for urlsafe, only_changed in ((False, False), (True, True)):
            decode_and_check(dst, src, payloads, mr, urlsafe, only_changed)
    finally:
        reset(src, dst)


TWICE = b"Cookie: v=" + base64.b64encode(base64.b64encode(b"the secret: admin:admin, twice encoded")) + b"; path=/\r\n"


def test_sources_frames_and_double_decoding(src, dst, third, tmp_path):
    payloads = [TWICE, b"plain", b"=", b"Authorization: Basic YWRtaW46YWRtaW4=\r\n"] + [t for t in tail_payloads(90, seed=33, mr=16) if t]
    path = str(tmp_path / "base64.pcap")
    K.write_udp_pcap(path, *B6.packed_image(payloads))
    try:
        reset(src, dst, third)
        n_pay, _ = src.load_pcap_frames(path, "udp")
        assert n_pay == len(payloads)
        once = decode_and_check(dst, src, payloads, 14)["payloads"]
        assert once[3] == b"Authorization: Basic admin:admin\r\n" and b"admin" not in once[0]
        # the decoded arena is a source like any other: into a third context, and back into the first
        twice = decode_and_check(third, dst, once, 14)["payloads"]
        assert twice[0] == b"Cookie: v=the secret: admin:admin, twice encoded; path=/\r\n"
        decode_and_check(src, third, twice, 4, urlsafe=True)
        check_arena(dst, dict(zip(("arena", "off", "len"), B6.packed_image(once))))           # what dst holds has stayed
        # ... and kmpgpu_load_decoded runs over a base64 result as over any arena
        res = src.load_decoded(dst)
        check_arena(src, DM.load_decoded(once))
        assert res["stats"] == DM.load_decoded(once)["stats"]
    finally:
        reset(src, dst, third)


def test_over_a_field_buffer_and_over_streams(src, dst, third):
    """the headers of every message (kmpgpu_load_fields) and the reassembled streams (kmpgpu_load_streams) as sources: what those
    contexts hold is downloaded, and dst is the model's decoding of exactly that"""
    cred = base64.b64encode(b"admin:admin")
    msgs = [b"GET /a HTTP/1.1\r\nHost: x\r\nAuthorization: Basic " + cred + b"\r\n\r\nbody " + cred,
            b"POST /b HTTP/1.1\r\nCookie: jwt=" + blob(np.random.default_rng(1), 90) + b"\r\n\r\n", b"not http at all " + cred,
            b"HTTP/1.1 200 OK\r\nX-Token: " + cred[:9], cred[9:] + b"\r\n\r\n"] * 20
    try:
        reset(src, dst, third)
        src.load_arena(K.HostArena.from_payloads(msgs))
        src.set_meta(meta_of_flows(np.arange(len(msgs)) // 5 % 7))
        third.load_fields(src, "headers")
        headers = payloads_of(third)
        assert headers[0].endswith(b"Basic " + cred + b"\r\n") or headers[0].endswith(b"Basic " + cred)
        mine = decode_and_check(dst, third, headers, 14)["payloads"]
        assert b"admin:admin" in mine[0] and b"admin:admin" not in headers[0]
        src.build_flows()
        third.load_streams(src, depth=1 << 16)
        streams = payloads_of(third)
        assert any(cred in s for s in streams)                      # the credential cut in two payloads is whole in its stream
        mine = decode_and_check(dst, third, streams, 14, only_changed=True)["payloads"]
        assert sum(b"X-Token: admin:admin" in s for s in mine) >= 1
    finally:
        reset(src, dst, third)


# ------------------------------------------------------------------------------------------------
# source offsets across and behind 2^32
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("placement", ["split", "edge", "behind"])
def test_high_offsets(src, dst, big_buffer, placement):
    rng = np.random.default_rng(41)
    payloads = [B6.random_payload(rng, int(L)) for L in rng.choice([0, 7, 16, 64, 200, 1500], 200)]
    k = 70
    payloads[k] = b". " + alpha(30) + b"== " + alpha(100, salt=3) + b"=" + filler(20) + alpha(1200, salt=5)       # runs on both sides of byte 48
    payloads[k - 1] = filler(13) + alpha(18) + b"="
    try:
        reset(src, dst)
        keep = attach_placed(src, payloads, None, placed_base(placement, payloads, k=k), big_buffer)
        for mr, urlsafe, only_changed in ((4, False, False), (16, True, True)):
            decode_and_check(dst, src, payloads, mr, urlsafe, only_changed)
        del keep
    finally:
        reset(src, dst)
        src.load_arena(*EMPTY)


# ------------------------------------------------------------------------------------------------
# dst: derived state rebuilt; rows in src's numbering
# ------------------------------------------------------------------------------------------------
def test_the_rule_the_feature_is_for(src, dst):
    pats = [b"admin:admin", b"Basic "]
    rules = [([0], []), ([1], [0])]
    payloads = [b"GET / HTTP/1.1\r\nAuthorization: Basic YWRtaW46YWRtaW4=\r\n\r\n", b"nothing here", b"admin:admin in the clear",
                b"Authorization: Basic Z3Vlc3Q6Z3Vlc3Q=\r\n", b"x=" + base64.b64encode(b"....admin:admin....")]
    try:
        reset(src, dst)
        for m in (src, dst):
            m.set_patterns(pats); m.set_rules(rules)
        src.load_arena(K.HostArena.from_payloads(payloads))
        decoded = decode_and_check(dst, src, payloads, 14)["payloads"]
        assert decoded[0] == b"GET / HTTP/1.1\r\nAuthorization: Basic admin:admin\r\n\r\n" and decoded[3].endswith(b"Basic guest:guest\r\n")
        for m, texts, fires in ((dst, decoded, [True, False, True, False, True]), (src, payloads, [False, False, True, False, False])):
            hits = MM.hits(MM.starts(texts, pats))
            res = check_rules(m, hits, rules, MM.counts(MM.starts(texts, pats)))
            assert res["hits"][0].tolist() == fires                                  # rows and any[] in src's numbering
            assert m.scan_packets()["any"].tolist() == hits.any(axis=0).tolist()
    finally:
        reset(src, dst)


def test_dst_state_every_family(src, dst, oracle):
    """patterns with nocase flags, rules, byte tests and expressions set on dst BEFORE the call, an arena of its own first: fold,
    bitmap and plans are made again for the decoded arena; the metadata handed on carries the flows"""
    rng = np.random.default_rng(51)
    words = [b"/admin", b"../", b"<script", b"select", b"GET ", b"a b"]
    payloads = []
    for k in range(400):
        parts = [plain(rng, int(rng.integers(0, 40))).replace(b"\0", b"q")]
        for _ in range(int(rng.integers(0, 4))):
            w = words[int(rng.integers(0, len(words)))]
            if rng.random() < 0.3:
                w = w.swapcase()
            if rng.random() < 0.6:
                w = b" " + base64.b64encode(b"0123456789"[:int(rng.integers(4, 10))] + w + b"!?") + b" "
            parts += [w, plain(rng, int(rng.integers(0, 300))).replace(b"\0", b"q")]
        payloads.append(b"".join(parts))
    pats = [b"/admin", b"../", b"<SCRIPT", b"select", b"GET "]
    nocase = [False, False, True, True, False]
    tests = [BM.bt(1, BM.EQ, 0x2F, 4), BM.isdataat(40)]
    exprs = [b"a b", RX.rx(b"/[a-z]+/\\.\\./", nocase=True), RX.rx(b"adm[i1]n", gate=0)]
    np_ = len(pats)
    rules = [([0], []), ([1, 4], []), ([2], [3]), ([np_ + 0], [np_ + 1]), ([np_ + 2], []), ([np_ + 4], [0])]
    meta = meta_of_flows(np.arange(len(payloads)) // 5 % 31)
    try:
        reset(src, dst)
        src.set_patterns(pats[:2], nocase=[True, False])
        dst.set_patterns(pats, nocase=nocase); dst.set_bytetests(tests); dst.set_regexes(exprs); dst.set_rules(rules)
        dst.load_arena(K.HostArena.from_payloads(payloads[:40]))                    # an arena, a fold and plans of its own first
        assert dst.scan()[0].tolist() == MM.oracle_counts(oracle, payloads[:40], pats, nocase)
        src.load_arena(K.HostArena.from_payloads(payloads))
        src.set_meta(meta)
        before = src.scan_packets(hits=True)
        mine = decode_and_check(dst, src, payloads, 12)["payloads"]
        st = MM.starts(mine, pats, None, nocase)
        hits, counts = MM.hits(st, np_), MM.oracle_counts(oracle, mine, pats, nocase)
        assert counts != MM.oracle_counts(oracle, payloads, pats, nocase)
        check_packets(dst, hits, counts)
        brows = BM.bytetest_rows(mine, pats, tests, None, nocase, False, st)
        xrows = RX.regex_rows(mine, exprs, False, hits)
        assert np.array_equal(dst.scan_bytetests(hits=True)["hits"], brows)
        assert np.array_equal(dst.scan_regexes(hits=True)["hits"], xrows)
        assert xrows[0].any() and hits.any()
        mat = np.concatenate([hits, brows, xrows])
        check_rules(dst, mat, rules, counts)
        assert dst.meta().tobytes() == meta.tobytes()
        dst.build_flows()
        fo = FM.flow_of_np(meta)
        check_fold(dst, "rules", "flow", FM.flow_rules(mat, fo, rules), counts)
        after = src.scan_packets(hits=True)
        assert all(np.array_equal(before[f], after[f]) for f in ("hits", "any", "pkt_counts", "counts"))
        # a small decode into the same context leaves nothing of the large one behind
        src.load_arena(K.HostArena.from_payloads(payloads[7:12]))
        mine = decode_and_check(dst, src, payloads[7:12], 12)["payloads"]
        check_packets(dst, MM.hits(MM.starts(mine, pats, None, nocase), np_), MM.oracle_counts(oracle, mine, pats, nocase))
    finally:
        reset(src, dst)
        dst.set_patterns([b"x"])                                                     # drops rules, byte tests and expressions


# ------------------------------------------------------------------------------------------------
# life cycle and errors, through the raw ABI
# ------------------------------------------------------------------------------------------------
def test_life_cycle_and_errors(src, dst):
    g = _lib.gpu_lib()
    payloads = mix(200, lambda k: k % 5 == 0)
    kept = mix(77, lambda k: False)
    want_kept = dict(zip(("arena", "off", "len"), B6.packed_image(kept)))
    st = _lib.DecodeStats()
    d_changed = C.c_void_p()
    words = np.zeros(8, dtype=np.uint64)

    def call(d, s, min_run=16, flags=0):
        st.n_payloads = 12345
        d_changed.value = 1
        return g.kmpgpu_load_base64(d, s, min_run, flags, words.ctypes.data, C.byref(d_changed), C.byref(st))

    def dst_keeps_its_arena(rc, code, what):
        assert rc == code, (rc, code)
        msg = g.kmpgpu_last_error()
        assert b"kmpgpu_load_base64" in msg and what in msg, msg
        assert st.n_payloads == 0 and not d_changed.value
        check_arena(dst, want_kept)

    try:
        reset(src, dst)
        src.load_arena(K.HostArena.from_payloads(payloads))
        dst.load_arena(K.HostArena.from_payloads(kept))
        dst_keeps_its_arena(call(dst._ctx, dst._ctx), EINVAL, b"same context")
        dst_keeps_its_arena(call(None, src._ctx), EINVAL, b"ctx is NULL")
        dst_keeps_its_arena(call(dst._ctx, None), EINVAL, b"ctx is NULL")
        for bad in (0, 3, 256, 0xFFFFFFFF):
            dst_keeps_its_arena(call(dst._ctx, src._ctx, min_run=bad), EINVAL, b"min_run %d is outside 4..255" % bad)
        dst_keeps_its_arena(call(dst._ctx, src._ctx, flags=4), EINVAL, b"flag bits")
        dst_keeps_its_arena(call(dst._ctx, src._ctx, flags=0x80000001), EINVAL, b"flag bits")
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
                n_pay = C.c_uint64()
                assert g.kmpgpu_load_frames_finish(other._ctx, C.byref(n_pay)) == 0
        finally:
            _lib.host_lib().kmp_frames_free(C.byref(fr))
        # src without an arena: dst empty, nothing handed out
        src.load_arena(*EMPTY)
        assert call(dst._ctx, src._ctx, flags=B64_URLSAFE) == 0
        assert dst.arena_info() == (0, 0) and st.n_payloads == 0 and not d_changed.value
        res = dst.load_base64(src)
        assert res["changed"].shape == (0,) and res["index"].shape == (0,) and res["stats"]["n_payloads"] == 0
        # NULL outputs, and a decode after the empty one with its timing
        src.load_arena(K.HostArena.from_payloads(payloads))
        assert g.kmpgpu_load_base64(dst._ctx, src._ctx, 16, 0, None, None, None) == 0
        check_arena(dst, B6.load_base64(payloads))
        assert dst.last_timing().launches == LAUNCHES
        decode_and_check(dst, src, payloads, 16, True, True)
    finally:
        reset(src, dst)


def test_two_devices_are_refused(src):
    if device_count() < 2:
        pytest.skip("one device")
    g = _lib.gpu_lib()
    with GpuMatcher(1) as far:
        src.load_arena(K.HostArena.from_payloads([b"QUJDREVGR0hJSktM", b"", b"x" * 40]))
        assert g.kmpgpu_load_base64(far._ctx, src._ctx, 16, 0, None, None, None) == EINVAL
        assert b"kmpgpu_load_base64" in g.kmpgpu_last_error() and far.arena_info() == (0, 0)


# ------------------------------------------------------------------------------------------------
# the command lines: KMPGPU_BASE64
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prog, extra", [("serial", ()), ("openmp_data", ("1",))])
def test_command_lines(tmp_path, prog, extra):
    """the row outputs are decided on the base64-decoded payloads, stdout stays the report over the payloads as captured"""
    jwt = base64.urlsafe_b64encode(b'{"user":"\xff","admin":true}').rstrip(b"=")
    assert b"_" in jwt and len(jwt.split(b"_")[1]) >= 14       # without ,url the run behind the '_' starts off a group of four
    payloads = [b"GET / HTTP/1.1\r\nAuthorization: Basic YWRtaW46YWRtaW4=\r\n\r\n", b"Cookie: jwt=" + jwt + b"\r\n", b"admin:admin as it is",
                b"q=a b&x=1", b"nothing to see here"]
    pats = [b"admin:admin", b'"admin":true', b"Basic"]
    exprs = [b"a b"]
    rules = [([0], []), ([1], []), ([3], []), ([2], [0, 1])]                       # term 3: the expression
    pcap, strings, rf, xf = (str(tmp_path / name) for name in ("base64.pcap", "patterns.txt", "rules.txt", "expressions.txt"))
    K.write_udp_pcap(pcap, *B6.packed_image(payloads))
    with open(strings, "wb") as f:
        f.write(b" ".join(pats) + b"\n")
    with open(rf, "w") as f:
        f.write("0\n1\nx0\n2 !0 !1\n")
    with open(xf, "w") as f:
        f.write("/a b/\n")
    meta = K.HostArena.from_pcap(pcap, "udp", with_meta=True).meta
    fo = FM.flow_of_np(meta)
    raw_report = K.format_report(pats, MM.counts(MM.starts(payloads, pats)))
    seen = {}
    for value in (None, "14", "14,url"):
        texts = payloads if value is None else [B6.decode(t, 14, value.endswith("url")) for t in payloads]
        hits = MM.hits(MM.starts(texts, pats))
        mat = np.concatenate([hits, RX.regex_rows(texts, exprs, False, hits)])
        rows = MM.rule_rows(mat, rules)
        out = {name: tmp_path / f"{name}_{value}.csv" for name in ("packets", "alerts", "flow_alerts", "flows")}
        env = {"KMPGPU_RULES_FILE": rf, "KMPGPU_REGEX_FILE": xf, "KMPGPU_PACKETS_FILE": str(out["packets"]), "KMPGPU_ALERTS_FILE": str(out["alerts"]),
               "KMPGPU_FLOW_ALERTS_FILE": str(out["flow_alerts"]), "KMPGPU_FLOWS_FILE": str(out["flows"])}
        if value:
            env["KMPGPU_BASE64"] = value
        r = run_cli(prog, pcap=pcap, strings=strings, extra=extra, env_extra=env)
        assert r.returncode == 0, r.stderr
        assert strip_elapsed(r.stdout) == raw_report                                # byte for byte what it is without the variable
        assert out["packets"].read_text() == "".join(f"{k},{i}\n" for k in range(len(payloads)) for i in range(len(pats)) if hits[i, k])
        assert out["alerts"].read_text() == "".join(f"{k},{q}\n" for k in range(len(payloads)) for q in range(len(rules)) if rows[q, k])
        assert out["flow_alerts"].read_text() == FM.flow_alerts_file(FM.flow_rules(mat, fo, rules))
        seen[value] = {name: path.read_text() for name, path in out.items()}
    assert seen[None]["flows"] == seen["14"]["flows"] == seen["14,url"]["flows"] != ""
    assert "0,0\n" not in seen[None]["alerts"] and "0,0\n" in seen["14"]["alerts"] and "0,0\n" in seen["14,url"]["alerts"]
    assert "1,1\n" not in seen["14"]["alerts"] and "1,1\n" in seen["14,url"]["alerts"]
