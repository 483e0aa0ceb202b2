"""kmpgpu_load_decoded (GpuMatcher.load_decoded) on a real MI355X: the payloads of a context percent-decoded on the device into a
packed arena that a second context owns, compared with tests/decode_model.py exactly -- arena bytes including the zero padding,
offsets, lengths, the changed bitmap with the bits at n and above 0, the stats and the index.

Where the kernels of csrc/kmp_decode.hip take another path:
  an escape straddling two 16-byte units (two lanes) or two steps of 64 units (lane 63 / lane 0)      test_boundaries
  an escape that ends at the payload's end, an incomplete one at L - 2 and L - 1                       test_boundaries
  a step without an escape at a 16-byte aligned output position (the straight copy) / any other one    test_densities
  a step with a '%' in it and no escape: the neighbours are asked, and the step is still copied        test_densities[lone_percent]
  runs of 64 payloads and a rest                                                                      test_densities[64 bytes]
  nothing behind a payload's end decodes: dirty padding, the next slot, the arena's end                test_sources_*
  source offsets across and behind 2^32                                                               test_high_offsets
  destination offsets as 64-bit values, > 4 GiB                           tests/test_gpu_high_destinations.py::test_decoded_past_2_32
Past the grid caps: tests/test_gpu_decode_scale.py.

No test provokes a fault: every negative case is one the library refuses on the host before it launches anything.

Run on a real MI355X:  python -m pytest tests/test_gpu_decode.py -m gpu
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

import bytetest_model as BM  # noqa: E402
import decode_model as DM  # noqa: E402
import flow_model as FM  # noqa: E402
import match_model as MM  # noqa: E402
import multithreading_string_matching_amd as K  # noqa: E402
import regex_model as RX  # noqa: E402
from multithreading_string_matching_amd import _lib  # noqa: E402
from multithreading_string_matching_amd.matcher import (  # noqa: E402
    DECODE_ONLY_CHANGED, DECODE_PERCENT, DECODE_PLUS, OPT_NONTEMPORAL, OPT_REPACK, OPT_WHOLE_PAYLOAD, GpuMatcher, device_count)

EINVAL, ESTATE = -2, -3
ONES = 0xFFFFFFFFFFFFFFFF
LAUNCHES = 5                      # kmpgpu.h: decoded lengths, two scan kernels, index, write
LAUNCHES_EMPTY = 3                # ... and where dst ends up without a payload
EMPTY = (np.zeros(0, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint32))
MODES = [(False, False), (True, False), (False, True), (True, True)]            # (plus, only_changed)


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


def decode_and_check(dst, src, payloads, plus=False, only_changed=False):
    want = DM.load_decoded(payloads, plus, only_changed)
    res = dst.load_decoded(src, plus=plus, only_changed=only_changed)
    assert first_diff(res["changed"], want["changed"]) is None, first_diff(res["changed"], want["changed"])
    assert np.array_equal(res["index"], want["index"]) and res["index"].dtype == np.int64
    assert res["stats"] == want["stats"]
    check_arena(dst, want)
    t = dst.last_timing()
    assert t.launches == (LAUNCHES if want["payloads"] else LAUNCHES_EMPTY) and t.kernel_ms > 0
    return want


def filler(L, salt=0):
    """bytes without a '%': hex digits, so that what lies next to an incomplete escape could complete it, a '+', others"""
    base = b"0a9Fx+g/Bc7 "
    return bytes(base[(i + salt) % len(base)] for i in range(L))


# ------------------------------------------------------------------------------------------------
# 5. boundaries
# ------------------------------------------------------------------------------------------------
BOUNDARY_LENGTHS = [0, 1, 2, 3, 15, 16, 17, 31, 32, 33, 1021, 1022, 1023, 1024, 1025, 1026, 1027, 2047, 2048, 2049, 2050, 9000]


def boundary_payloads():
    out = []
    for L in BOUNDARY_LENGTHS:
        out.append(filler(L, L))
        starts = {0, 1, 12, 13, 14, 15, 16, L - 4, L - 3, L - 2, L - 1, 1021, 1022, 1023, 1024}
        for i in sorted(s for s in starts if 0 <= s < L):
            b = bytearray(filler(L, L + i))
            esc = b"%%%02X" % ((i * 7 + L) & 0xFF)
            b[i:i + 3] = esc[:L - i]                   # at L - 2 and L - 1 what fits: an incomplete escape, which stays
            out.append(bytes(b))
    return out


@pytest.fixture(scope="module")
def boundaries():
    return boundary_payloads()


@pytest.mark.parametrize("plus, only_changed", MODES)
def test_boundaries(src, dst, boundaries, plus, only_changed):
    assert any(t.endswith(b"%") for t in boundaries) and any(t[-2:-1] == b"%" for t in boundaries if len(t) > 1)
    try:
        reset(src, dst)
        src.load_arena(K.HostArena.from_payloads(boundaries))
        want = decode_and_check(dst, src, boundaries, plus, only_changed)
        assert 0 < want["stats"]["n_changed"] < len(boundaries) or plus
    finally:
        reset(src, dst)


# ------------------------------------------------------------------------------------------------
# 6. densities
# ------------------------------------------------------------------------------------------------
def density_payloads(kind):
    rng = np.random.default_rng({"hostile": 1, "all_escaped": 2, "no_percent": 3, "64_bytes": 4, "lone_percent": 5}[kind])
    if kind == "lone_percent":
        # one run of 60 payloads of up to 80 bytes: a '%' in every unit, never two hex digits behind it, no '+'
        return [bytes(0x25 if j % 7 == 0 else 0x67 + (i + j) % 16 for j in range(int(L))) for i, L in enumerate(rng.integers(0, 81, 60))]
    if kind == "hostile":
        return [DM.random_payload(rng, int(L)) for L in rng.integers(0, 3001, 200)]
    if kind == "all_escaped":
        return [DM.escape_all(rng.integers(0, 256, int(L), dtype=np.uint8).tobytes()) for L in rng.integers(0, 1001, 200)]
    if kind == "no_percent":
        return [DM.random_payload(rng, int(L)).replace(b"%", b"x") for L in rng.integers(0, 3001, 200)]
    out = [DM.random_payload(rng, 64) for _ in range(130)]                        # two runs of 64 and a rest
    out[5], out[64], out[129] = filler(64), b"%41" * 21 + b"%", filler(62) + b"%4"
    return out


@pytest.mark.parametrize("kind", ["hostile", "all_escaped", "no_percent", "64_bytes", "lone_percent"])
def test_densities(src, dst, third, kind):
    payloads = density_payloads(kind)
    try:
        reset(src, dst, third)
        src.load_arena(K.HostArena.from_payloads(payloads))
        for plus, only_changed in MODES:
            want = decode_and_check(dst, src, payloads, plus, only_changed)
            if kind == "all_escaped":
                assert want["stats"]["bytes_in"] == 3 * want["stats"]["bytes_out"]
            if kind == "lone_percent":
                assert want["stats"]["n_changed"] == 0
        if kind == "no_percent":
            # nothing to decode: byte for byte what kmpgpu_load_selected with all bits set makes of the source
            dst.load_decoded(src)
            third.load_selected(src, np.ones(len(payloads), dtype=bool))
            assert all(np.array_equal(x, y) for x, y in zip(dst.arena_download(), third.arena_download()))
        # the other instantiation of the write kernel
        dst.set_option(OPT_NONTEMPORAL, 0)
        decode_and_check(dst, src, payloads, True, False)
    finally:
        reset(src, dst, third)


# ------------------------------------------------------------------------------------------------
# 7. KMPGPU_DECODE_ONLY_CHANGED, the device bitmap, the metadata
# ------------------------------------------------------------------------------------------------
def mix(n, which):
    rng = np.random.default_rng(n)
    out = []
    for k in range(n):
        t = DM.random_payload(rng, int(rng.integers(0, 200))).replace(b"%", b"y").replace(b"+", b"z")
        if which(k):
            t = t[:len(t) // 2] + b"%2e" + t[len(t) // 2:]
        out.append(t)
    return out


@pytest.mark.parametrize("name", ["every_third", "none", "all", "word_boundary"])
def test_only_changed(src, dst, third, name):
    n, which = {"every_third": (300, lambda k: k % 3 == 1), "none": (300, lambda k: False), "all": (300, lambda k: True),
                "word_boundary": (129, lambda k: k == 64)}[name]
    payloads = mix(n, which)
    meta = meta_of_flows(np.arange(n) // 4 % 23)
    g = _lib.gpu_lib()
    try:
        reset(src, dst, third)
        src.load_arena(K.HostArena.from_payloads(payloads))
        src.set_meta(meta)
        for only in (True, False):
            want = decode_and_check(dst, src, payloads, False, only)
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
        assert g.kmpgpu_load_decoded(dst._ctx, src._ctx, DECODE_PERCENT, DECODE_ONLY_CHANGED, words.ctypes.data, C.byref(d_changed), C.byref(st)) == 0
        assert np.array_equal(words, DM.words([which(k) for k in range(n)]))         # the bits at n and above are 0
        assert d_changed.value and st.n_payloads == st.n_changed == sum(which(k) for k in range(n))
        n_sel = C.c_uint64()
        assert g.kmpgpu_load_selected(third._ctx, src._ctx, d_changed, 1, C.byref(n_sel)) == 0 and n_sel.value == st.n_changed
        raw = [payloads[k] for k in range(n) if which(k)]
        check_arena(third, dict(zip(("arena", "off", "len"), DM.packed_image(raw))))
    finally:
        reset(src, dst, third)


# ------------------------------------------------------------------------------------------------
# 8. every kind of source
# ------------------------------------------------------------------------------------------------
def tail_payloads(n, seed):
    """every payload ends in '%4' or '%' (or is shorter), with escapes inside"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        L = int(rng.choice([0, 1, 2, 14, 15, 16, 17, 30, 31, 32, 100, 1023, 1024, 1500]))
        t = bytearray(DM.random_payload(rng, L))
        tail = (b"%4", b"%", b"%a", b"%")[k % 4]
        m = min(L, len(tail))
        t[L - m:] = tail[:m]
        out.append(bytes(t))
    return out


def test_sources_borrowed_with_dirty_padding(src, dst):
    """the padding holds hex digits: nothing behind a payload's end completes its last escape"""
    payloads = tail_payloads(600, seed=31)
    slots = [t + (b"1F" * 16)[:(-len(t)) % 16 or (0 if t else 16)] for t in payloads]
    assert sum(len(s) > len(t) for s, t in zip(slots, payloads)) > 400
    try:
        reset(src, dst)
        keep = attach_slots(src, payloads, slots)
        before = keep[0].cpu().numpy().copy()
        for plus, only_changed in MODES:
            decode_and_check(dst, src, payloads, plus, only_changed)
        assert np.array_equal(keep[0].cpu().numpy(), before)
    finally:
        reset(src, dst)
        src.load_arena(*EMPTY)


@pytest.mark.parametrize("repack", [0, 1])
def test_sources_with_gaps_and_shuffled_slots(src, dst, repack):
    rng = np.random.default_rng(32)
    payloads = tail_payloads(500, seed=32)
    ln = np.array([len(t) for t in payloads], dtype=np.int64)
    slot = np.maximum(16, (ln + 15) & ~15)
    order = rng.permutation(len(payloads))
    adv = 16 * rng.integers(0, 4, len(payloads)) + slot[order]
    off = np.zeros(len(payloads), dtype=np.int64)
    off[order] = np.cumsum(adv) - slot[order]
    arena = np.frombuffer((b"%41" * (int(adv.sum()) // 3 + 40))[:int(adv.sum()) + 64], dtype=np.uint8).copy()      # gaps and padding: escapes
    for o, t in zip(off, payloads):
        arena[int(o):int(o) + len(t)] = np.frombuffer(t, dtype=np.uint8)
    try:
        reset(src, dst)
        src.set_option(OPT_REPACK, repack)
        src.load_arena(arena, off.astype(np.uint64), ln.astype(np.uint32))
        if not repack:
            assert first_diff(src.arena_download()[1], off) is None            # not packed: the index is followed as it is
        for plus, only_changed in ((False, False), (True, True)):
            decode_and_check(dst, src, payloads, plus, only_changed)
    finally:
        reset(src, dst)


def test_sources_frames_and_double_decoding(src, dst, third, tmp_path):
    payloads = [b"GET /%252e%252e%252fetc/passwd", b"plain", b"%", b"%2541%25", b"a%2Bb+c%252B"] + [t for t in tail_payloads(90, seed=33) if t]
    path = str(tmp_path / "escapes.pcap")
    K.write_udp_pcap(path, *DM.packed_image(payloads))
    try:
        reset(src, dst, third)
        n_pay, _ = src.load_pcap_frames(path, "udp")
        assert n_pay == len(payloads)
        once = decode_and_check(dst, src, payloads)["payloads"]
        assert once[0] == b"GET /%2e%2e%2fetc/passwd" and once[3] == b"%41%"
        # the decoded arena is a source like any other: into a third context, and back into the first
        twice = decode_and_check(third, dst, once)["payloads"]
        assert twice[0] == b"GET /../etc/passwd" and twice[3] == b"A%"
        decode_and_check(src, third, twice, plus=True)
        check_arena(dst, dict(zip(("arena", "off", "len"), DM.packed_image(once))))           # what dst holds has stayed
    finally:
        reset(src, dst, third)


@pytest.mark.parametrize("tail", [b"%", b"%4"])
def test_sources_arena_tight_at_the_last_slot(src, dst, tail):
    payloads = [b"%41" * 5, b"x" * 31, b"", (b"0123456789abcdef" * 3)[:48 - len(tail)] + tail]
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
        for plus, only_changed in MODES:
            decode_and_check(dst, src, payloads, plus, only_changed)
    finally:
        reset(src, dst)
        src.load_arena(*EMPTY)


# ------------------------------------------------------------------------------------------------
# 9. source offsets across and behind 2^32
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("placement", ["split", "edge", "behind"])
def test_high_offsets(src, dst, big_buffer, placement):
    rng = np.random.default_rng(41)
    payloads = [DM.random_payload(rng, int(L)) for L in rng.choice([0, 7, 16, 64, 200, 1500], 200)]
    k = 70
    payloads[k] = (b"%41%42" + filler(34) + b"%2e%2E" + b"%2f" + filler(3) + b"%30" * 40 + filler(50) + b"%")      # escapes on both sides of byte 48
    payloads[k - 1] = filler(29) + b"%4A"
    try:
        reset(src, dst)
        keep = attach_placed(src, payloads, None, placed_base(placement, payloads, k=k), big_buffer)
        for plus, only_changed in ((False, False), (True, True)):
            decode_and_check(dst, src, payloads, plus, only_changed)
        del keep
    finally:
        reset(src, dst)
        src.load_arena(*EMPTY)


# ------------------------------------------------------------------------------------------------
# 10. dst: derived state rebuilt, buffers reused; src: untouched
# ------------------------------------------------------------------------------------------------
def test_the_evasion_the_feature_is_for(src, dst):
    """In dst the rules fire on the first three payloads under the default text rule -- the decoded 0x00 of the fourth ends its text --
    and on all four under KMPGPU_OPT_WHOLE_PAYLOAD.  In src they fire on the third and the fourth under either rule: the fourth
    carries a raw `/admin` behind its `%00`, and the three bytes `%00` are no 0x00, so nothing ends its text (tests/match_model.py
    decides every expectation here)."""
    pats = [b"/admin", b"../"]
    rules = [([0], []), ([1], []), ([], [0, 1])]
    payloads = [b"GET /%61dmin", b"GET /%2e%2e%2fetc", b"GET /admin", b"GET /a%00/admin"]
    try:
        reset(src, dst)
        for m in (src, dst):
            m.set_patterns(pats); m.set_rules(rules)
        src.load_arena(K.HostArena.from_payloads(payloads))
        decoded = decode_and_check(dst, src, payloads)["payloads"]
        assert decoded == [b"GET /admin", b"GET /../etc", b"GET /admin", b"GET /a\0/admin"]
        for whole, in_dst, in_src in ((0, [True, True, True, False], [False, False, True, True]),
                                      (1, [True, True, True, True], [False, False, True, True])):
            for m, texts, fires in ((dst, decoded, in_dst), (src, payloads, in_src)):
                m.set_option(OPT_WHOLE_PAYLOAD, whole)
                hits = MM.hits(MM.starts(texts, pats, whole=bool(whole)))
                res = check_rules(m, hits, rules, MM.counts(MM.starts(texts, pats, whole=bool(whole))))
                assert (res["hits"][0] | res["hits"][1]).tolist() == fires
    finally:
        reset(src, dst)


def test_dst_state_every_family(src, dst, oracle):
    """patterns with nocase flags, rules, byte tests and expressions set on dst BEFORE the call, an arena of its own first: fold,
    bitmap and plans are made again for the decoded arena; the metadata handed on carries the flows"""
    rng = np.random.default_rng(51)
    words = [b"/admin", b"../", b"<script", b"select", b"GET ", b"a b"]
    payloads = []
    for k in range(400):
        parts = [DM.random_payload(rng, int(rng.integers(0, 40))).replace(b"\0", b"q")]
        for _ in range(int(rng.integers(0, 4))):
            w = words[int(rng.integers(0, len(words)))]
            if rng.random() < 0.6:
                w = b"".join(b"%%%02x" % c if rng.random() < 0.5 else bytes([c]) for c in w)
            if rng.random() < 0.3:
                w = w.swapcase()
            parts += [w, DM.random_payload(rng, int(rng.integers(0, 300)))]
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
        for plus in (False, True):
            mine = decode_and_check(dst, src, payloads, plus)["payloads"]
            st = MM.starts(mine, pats, None, nocase)
            hits, counts = MM.hits(st, np_), MM.oracle_counts(oracle, mine, pats, nocase)
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
        mine = decode_and_check(dst, src, payloads[7:12])["payloads"]
        check_packets(dst, MM.hits(MM.starts(mine, pats, None, nocase), np_), MM.oracle_counts(oracle, mine, pats, nocase))
    finally:
        reset(src, dst)
        dst.set_patterns([b"x"])                                                     # drops rules, byte tests and expressions


# ------------------------------------------------------------------------------------------------
# 11. life cycle and errors, through the raw ABI
# ------------------------------------------------------------------------------------------------
def test_life_cycle_and_errors(src, dst):
    g = _lib.gpu_lib()
    payloads = mix(200, lambda k: k % 5 == 0)
    kept = mix(77, lambda k: False)
    want_kept = dict(zip(("arena", "off", "len"), DM.packed_image(kept)))
    st = _lib.DecodeStats()
    d_changed = C.c_void_p()
    words = np.zeros(8, dtype=np.uint64)

    def call(d, s, transform=DECODE_PERCENT, flags=0):
        st.n_payloads = 12345
        d_changed.value = 1
        return g.kmpgpu_load_decoded(d, s, transform, flags, words.ctypes.data, C.byref(d_changed), C.byref(st))

    def dst_keeps_its_arena(rc, code, what):
        assert rc == code, (rc, code)
        msg = g.kmpgpu_last_error()
        assert b"kmpgpu_load_decoded" in msg and what in msg, msg
        assert st.n_payloads == 0 and not d_changed.value
        check_arena(dst, want_kept)

    try:
        reset(src, dst)
        src.load_arena(K.HostArena.from_payloads(payloads))
        dst.load_arena(K.HostArena.from_payloads(kept))
        dst_keeps_its_arena(call(dst._ctx, dst._ctx), EINVAL, b"same context")
        dst_keeps_its_arena(call(None, src._ctx), EINVAL, b"ctx is NULL")
        dst_keeps_its_arena(call(dst._ctx, None), EINVAL, b"ctx is NULL")
        dst_keeps_its_arena(call(dst._ctx, src._ctx, transform=0), EINVAL, b"transform 0")
        dst_keeps_its_arena(call(dst._ctx, src._ctx, transform=2), EINVAL, b"transform 2")
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
        assert call(dst._ctx, src._ctx, flags=DECODE_PLUS) == 0
        assert dst.arena_info() == (0, 0) and st.n_payloads == 0 and not d_changed.value
        res = dst.load_decoded(src)
        assert res["changed"].shape == (0,) and res["index"].shape == (0,) and res["stats"]["n_payloads"] == 0
        # NULL outputs, and a decode after the empty one with its timing
        src.load_arena(K.HostArena.from_payloads(payloads))
        assert g.kmpgpu_load_decoded(dst._ctx, src._ctx, DECODE_PERCENT, 0, None, None, None) == 0
        check_arena(dst, DM.load_decoded(payloads))
        assert dst.last_timing().launches == LAUNCHES
        decode_and_check(dst, src, payloads, True, True)
    finally:
        reset(src, dst)


def test_two_devices_are_refused(src):
    if device_count() < 2:
        pytest.skip("one device")
    g = _lib.gpu_lib()
    with GpuMatcher(1) as far:
        src.load_arena(K.HostArena.from_payloads([b"%41", b"", b"x" * 40]))
        assert g.kmpgpu_load_decoded(far._ctx, src._ctx, DECODE_PERCENT, 0, None, None, None) == EINVAL
        assert b"kmpgpu_load_decoded" in g.kmpgpu_last_error() and far.arena_info() == (0, 0)


# ------------------------------------------------------------------------------------------------
# 13. the command lines: KMPGPU_DECODE
# ------------------------------------------------------------------------------------------------
from gpu_support import run_cli, strip_elapsed  # noqa: E402


@pytest.mark.parametrize("prog, extra", [("serial", ()), ("openmp_data", ("1",))])
def test_command_lines(tmp_path, prog, extra):
    """the row outputs are decided on the decoded payloads, stdout stays the report over the payloads as captured"""
    payloads = [b"GET /%61dmin HTTP/1.1", b"GET /%2e%2e%2fetc/passwd", b"GET /admin", b"q=a+b&x=1", b"nothing to see here"]
    pats = [b"/admin", b"../", b"GET"]
    exprs = [b"a b"]
    rules = [([0], []), ([1], []), ([3], []), ([2], [0, 1])]                       # term 3: the expression
    pcap, strings, rf, xf = (str(tmp_path / name) for name in ("escapes.pcap", "patterns.txt", "rules.txt", "expressions.txt"))
    K.write_udp_pcap(pcap, *DM.packed_image(payloads))
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
    for value in (None, "percent", "percent+plus"):
        texts = payloads if value is None else [DM.decode(t, plus=value.endswith("plus")) for t in payloads]
        hits = MM.hits(MM.starts(texts, pats))
        mat = np.concatenate([hits, RX.regex_rows(texts, exprs, False, hits)])
        rows = MM.rule_rows(mat, rules)
        out = {name: tmp_path / f"{name}_{value}.csv" for name in ("packets", "alerts", "flow_alerts", "flows")}
        env = {"KMPGPU_RULES_FILE": rf, "KMPGPU_REGEX_FILE": xf, "KMPGPU_PACKETS_FILE": str(out["packets"]), "KMPGPU_ALERTS_FILE": str(out["alerts"]),
               "KMPGPU_FLOW_ALERTS_FILE": str(out["flow_alerts"]), "KMPGPU_FLOWS_FILE": str(out["flows"])}
        if value:
            env["KMPGPU_DECODE"] = value
        r = run_cli(prog, pcap=pcap, strings=strings, extra=extra, env_extra=env)
        assert r.returncode == 0, r.stderr
        assert strip_elapsed(r.stdout) == raw_report                                # byte for byte what it is without the variable
        assert out["packets"].read_text() == "".join(f"{k},{i}\n" for k in range(len(payloads)) for i in range(len(pats)) if hits[i, k])
        assert out["alerts"].read_text() == "".join(f"{k},{q}\n" for k in range(len(payloads)) for q in range(len(rules)) if rows[q, k])
        assert out["flow_alerts"].read_text() == FM.flow_alerts_file(FM.flow_rules(mat, fo, rules))
        seen[value] = {name: path.read_text() for name, path in out.items()}
    assert seen[None]["flows"] == seen["percent"]["flows"] == seen["percent+plus"]["flows"] != ""
    assert "0,0\n" not in seen[None]["alerts"] and "0,0\n" in seen["percent"]["alerts"] and "1,1\n" in seen["percent"]["alerts"]
    assert "3,2\n" not in seen["percent"]["alerts"] and "3,2\n" in seen["percent+plus"]["alerts"]
