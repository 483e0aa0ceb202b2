"""Byte tests on the GPU (kmpgpu_set_bytetests / kmpgpu_scan_bytetests, include/kmpgpu.h) against tests/bytetest_model.py, exactly: an
independent model in plain Python, held to hand-written answers by tests/test_bytetest_model.py.

One synthetic capture is shared.  Its bytes come from a small alphabet (with 0x00 at chosen and at random places), so that a compare
on a field splits the payloads; every test asserts on the model's rows that none under test is trivially empty or full -- apart from the
ones named as such -- before it looks at the device's.
"""
import os

import numpy as np
import pytest

from conftest import DATA, GOLDEN

from gpu_support import KERNELS, check_fold, gm, load, meta_of_flows, reset, run_cli, strip_elapsed, torch  # noqa: F401  (gm: the context fixture)

import bytetest_model as BM
import flow_model as FM
import header_model as HM
import match_model as MM
from bytetest_model import EQ, GE, GT, LE, LT, NE, bt
from multithreading_string_matching_amd import _lib
from multithreading_string_matching_amd._lib import KmpGpuError
from multithreading_string_matching_amd.host import BYTETEST_DTYPE, HostArena
from multithreading_string_matching_amd.matcher import OPT_FUSED, OPT_KERNEL, OPT_REPACK, OPT_WHOLE_PAYLOAD, GpuMatcher

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -2, -3
BT_TILE = _lib.BT_TILE        # tests the absolute kernel stages at a time
U32 = 0xFFFFFFFF
ONES = U32 << 32 | U32
N_MAX = 4097
LENS = [0, 1, 3, 4, 5, 15, 16, 17, 40, 1500]
ALPHA = bytes([1, 2, 3, 4, 0x7F, 0x80, 0xFF, 0x41, 0x61, 0x3A])
PATS = [b"LEN:", b"id", b"key="]
NOCASE = [False, True, False]

# the hand cases of tests/test_bytetest_model.py, planted as payloads 0 .. 12
PLANTED = [bytes([1, 2, 3, 4]), bytes([0x80, 0, 0, 0, 1]), b"A", b"abcd", b"ab\0cd", b"", b"\x07", b"\x07\x08\x09", b"\x07\x08\x09\x0a",
           b"xxLEN:\x01\x02yy", b"LEN:\x01\x01 LEN:\x09\x09", b"iD:AB", b"\0abc"]


def raises(code, text):
    return pytest.raises(KmpGpuError, match=rf"\({code}\).*{text}")


# ------------------------------------------------------------------------------------------------
# the capture and the test lists
# ------------------------------------------------------------------------------------------------
def _capture(n, seed=5):
    rng = np.random.default_rng(seed)
    lens = rng.choice(LENS, n)
    out = []
    for k in range(n):
        L = int(lens[k])
        b = bytearray(rng.choice(np.frombuffer(ALPHA, dtype=np.uint8), L).tobytes())
        for z in np.flatnonzero(rng.integers(0, 40, L) == 0):          # 0x00 at random places (every fourth payload keeps none:
            if k % 4 != 1:                                             # a long text under the strlen rule) ...
                b[int(z)] = 0
        if L >= 15 and k % 3 == 0 and k % 4 != 1:                                     # ... and at chosen ones: byte 13 / byte 16 of every third
            b[13 if k % 2 else min(16, L - 1)] = 0
        if L >= 15:                                                    # anchors, each with two field bytes behind it
            for _ in range(1 + L // 200):
                word = [b"LEN:", b"id", b"ID", b"iD", b"key="][int(rng.integers(5))]
                at = int(rng.integers(0, L - len(word) - 1))
                b[at:at + len(word)] = word
        out.append(bytes(b))
    out[:len(PLANTED)] = PLANTED[:n]
    return out


# the fixed list; NEVER and WHOLE_ONLY below name the rows that are empty by design
FIXED = [
    bt(4, EQ, 0x01020304, 0),                              # payload 0, the only test of the lists of one
    bt(2, GT, 0x0800, 0, anchor=0),                        # relative and absolute tests take turns: the two kernels' rows interleave
    bt(4, EQ, 0x04030201, 0, little=True),
    bt(2, EQ, 0x4142, 1, anchor=1),                        # a nocase anchor, the field's letters in their own case
    bt(4, GT, 1, 0),                                       # unsigned across the top bit
    bt(1, EQ, 0x3A, -1, anchor=0),                         # into the match
    bt(1, EQ, 0, 0, mask=0),                               # mask 0: true wherever there is a byte
    bt(1, GE, 0x41, -5, anchor=0),                         # in front of the match
    bt(2, GE, 0x0203, 1),                                  # pos & 3 == 1, inside a dword
    bt(2, LT, 0x7F00, 2, anchor=2, little=True),
    bt(2, GE, 0x0304, 2),                                  # pos & 3 == 2
    bt(3, NE, 0x010101, 0, anchor=0, mask=0x0F0F0F),
    bt(2, LE, 0x7FFF, 3),                                  # pos & 3 == 3: across two dwords
    bt(1, GE, 0, 10, anchor=1),                            # isdataat behind an anchor
    bt(4, LT, 0x80000000, 1),                              # 4 bytes at 1 .. 3: two dwords
    bt(4, NE, 0, -4, anchor=0, mask=0x80808080),           # the anchor's own bytes: "LEN:" has no top bit set, never true
    bt(4, GE, 0x04000000, 2, little=True),
    bt(4, GT, 0x7F7F7F7F, 3),
    bt(3, GE, 0x7F0000, 14),                               # across a 16-byte unit: bytes 14 .. 16
    bt(4, LE, 0x80000000, 13, little=True),                # ... 13 .. 16
    bt(2, NE, 0, 15, mask=0x8080),                         # ... 15, 16
    bt(4, GT, 0x02000000, 12),                             # ends with the unit
    bt(3, EQ, 0x020304, 1), bt(3, EQ, 0x040302, 1, little=True),
    BM.isdataat(0), BM.isdataat(3), BM.isdataat(4), BM.isdataat(15), BM.isdataat(16), BM.isdataat(39), BM.isdataat(1499),
    BM.isdataat(1500),                                     # behind the longest payload: never true
    bt(2, NE, 0, 2, mask=0x8000),                          # the QR bit
    bt(2, EQ, 0x6200, 1), bt(1, EQ, 0x63, 3), bt(1, EQ, 0, 2),      # payload 4 under whole payloads: a 0x00 in, in front of, as the field
    bt(4, GE, 0, 1496),                                    # ends with the longest payload
    bt(2, GE, 0x0101, 0, anchor=0), bt(2, GE, 0x0101, 0, anchor=0),  # a duplicate: a row each
]
NEVER = {15, 31}                                           # rows that are empty by design
WHOLE_ONLY = {33, 34, 35}                                  # rows that need a byte at or behind a 0x00


def _drawn(rng):
    if rng.integers(3) == 0:
        return bt(int(rng.integers(1, 5)), int(rng.integers(6)), int(rng.choice([0, 1, 0x41, 0x7F, 0x80, 0x0102, 0x7F00, 0x800000, 0x01020304, 0x80000000])),
                  int(rng.choice([-6, -4, -2, -1, 0, 1, 2, 3, 10])), mask=int(rng.choice([U32, U32, 0xFF, 0x80808080])), anchor=int(rng.integers(3)),
                  little=bool(rng.integers(2)))
    return bt(int(rng.integers(1, 5)), int(rng.integers(6)), int(rng.choice([0, 1, 0x41, 0x7F, 0x80, 0x0102, 0x7F00, 0x800000, 0x01020304, 0x80000000])),
              int(rng.choice([0, 1, 2, 3, 5, 11, 12, 13, 14, 15, 16, 17, 36, 38, 1495])), mask=int(rng.choice([U32, U32, 0xFF, 0x80808080])),
              little=bool(rng.integers(2)))


def _tests(n, payloads):
    """n tests: the fixed list, then draws, kept where the model's row over the whole capture is neither empty nor full under either rule"""
    out = list(FIXED)
    rng = np.random.default_rng(17)
    st = {w: MM.starts(payloads, PATS, None, NOCASE, w) for w in (False, True)}
    while len(out) < n:
        cand = [_drawn(rng) for _ in range(32)]
        rows = [BM.bytetest_rows(payloads, PATS, cand, None, NOCASE, w, st[w]) for w in (False, True)]
        for q, t in enumerate(cand):
            if all(0 < r[q].sum() < len(payloads) for r in rows):
                out.append(t)
    return out[:n]


class World:
    def __init__(self):
        self.payloads = _capture(N_MAX)
        self.tests = _tests(BT_TILE + 1, self.payloads)
        self.st = {w: MM.starts(self.payloads, PATS, None, NOCASE, w) for w in (False, True)}
        self.rows = {w: BM.bytetest_rows(self.payloads, PATS, self.tests, None, NOCASE, w, self.st[w]) for w in (False, True)}
        self.relative = [q for q, t in enumerate(self.tests) if "anchor" in t]


@pytest.fixture(scope="module")
def world():
    w = World()
    assert len(w.tests) == BT_TILE + 1 and 20 < len(w.relative) < BT_TILE - 20
    assert ["anchor" in t for t in w.tests[:16]] == [False, True] * 8      # the two kernels' rows interleave
    n = len(w.payloads)
    for whole in (False, True):
        rows = w.rows[whole]
        for q in range(len(w.tests)):
            if q in NEVER or (not whole and q in WHOLE_ONLY):
                assert not rows[q].any(), (q, whole)
            else:
                assert 0 < rows[q].sum() < n, (q, whole, w.tests[q], int(rows[q].sum()))
    # the hand cases, bit by bit (payloads 0 .. 12; tests/test_bytetest_model.py spells the same answers out for the model)
    s, wh = w.rows[False], w.rows[True]
    assert s[0, 0] and s[2, 0] and not s[0, 1]                             # both byte orders of 01 02 03 04
    assert wh[4, 1] and not s[4, 1] and not s[4, 2]                        # 0x80000000 > 1 (under whole payloads: the field holds 0x00)
    assert s[6, 2] and not s[6, 5] and not s[6, 12] and wh[6, 12]          # mask 0: a byte is needed; payload 12 starts with 0x00
    assert s[22, 0] and s[23, 0]                                           # 3-byte fields
    assert s[1, 10] and not s[1, 9]                                        # the second match serves
    assert s[3, 11] and s[5, 9] and s[7, 9]                                # nocase anchor; into / in front of the match
    assert [bool(s[24, k]) for k in (5, 6, 7, 8)] == [False, True, True, True] and [bool(s[26, k]) for k in (7, 8)] == [False, False]
    assert [bool(s[25, k]) for k in (5, 6, 7, 8)] == [False, False, False, True]         # a field that ends exactly at E_k / one past it
    assert wh[33, 4] and wh[34, 4] and wh[35, 4] and not s[33, 4] and not s[34, 4] and not s[35, 4]
    assert s[37, 10] and s[38, 10] and np.array_equal(s[37], s[38])
    return w


def _not_trivial(rows):
    if rows.size == 1:
        assert rows.sum() == 1
    else:
        assert 0 < rows.sum() < rows.size


def _check(m, rows, counts=None):
    res = m.scan_bytetests(hits=True)
    bad = np.argwhere(res["hits"] != rows)
    assert bad.size == 0, [(int(q), int(k), bool(rows[q, k]), {f: int(m.bytetests[int(q)][f]) for f in BYTETEST_DTYPE.names}) for q, k in bad[:6]]
    assert res["bt_pkt_counts"].tolist() == rows.sum(axis=1).tolist()
    assert res["any"].tolist() == rows.any(axis=0).tolist()
    if counts is not None:
        assert res["counts"].tolist() == list(counts)
    return res


def _setup(m, payloads, tests, whole=False, slots=None):
    m.set_option(OPT_WHOLE_PAYLOAD, int(whole))
    m.set_patterns(PATS, nocase=NOCASE)
    keep = load(m, payloads, slots)
    m.set_bytetests(tests)
    return keep


# ------------------------------------------------------------------------------------------------
# 1. rows against the model
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("whole", [False, True])
@pytest.mark.parametrize("n_bt", [1, len(FIXED), BT_TILE + 1])
@pytest.mark.parametrize("n_pkts", [1, 63, 64, 65, 257, N_MAX])
def test_rows_against_the_model(gm, world, n_pkts, n_bt, whole):
    rows = world.rows[whole][:n_bt, :n_pkts]
    _not_trivial(rows)
    reset(gm)
    try:
        _setup(gm, world.payloads[:n_pkts], world.tests[:n_bt], whole)
        res = _check(gm, rows)
        # the marking pass, and one kernel per kind of test in the reduce's place
        plain = gm.scan_packets()
        kinds = len({"anchor" in t for t in world.tests[:n_bt]})
        assert res["timing"].launches == plain["timing"].launches - 1 + kinds
        assert res["counts"].tolist() == plain["counts"].tolist()
        # the raw words: the bits at n_pkts and above are 0
        W = (n_pkts + 63) // 64
        hit_w, any_w = np.full((n_bt, W), ONES, dtype=np.uint64), np.full(W, ONES, dtype=np.uint64)
        _lib.gpu_check(gm._g.kmpgpu_scan_bytetests(gm._ctx, None, any_w.ctypes.data, hit_w.ctypes.data, None, None), "kmpgpu_scan_bytetests")
        assert np.array_equal(hit_w, MM.words(rows)) and np.array_equal(any_w, MM.words(rows.any(axis=0)))
    finally:
        reset(gm)


@pytest.mark.parametrize("name,kernel,fused", KERNELS)
@pytest.mark.parametrize("whole", [False, True])
def test_every_streaming_kernel_selection(gm, world, oracle, whole, name, kernel, fused):
    n_pkts, n_bt = 1000, len(FIXED)
    rows = world.rows[whole][:n_bt, :n_pkts]
    _not_trivial(rows)
    counts = MM.oracle_counts(oracle, world.payloads[:n_pkts], PATS, NOCASE, whole)
    reset(gm)
    try:
        gm.set_option(OPT_KERNEL, kernel)
        gm.set_option(OPT_FUSED, fused)
        _setup(gm, world.payloads[:n_pkts], world.tests[:n_bt], whole)
        _check(gm, rows, counts)
    finally:
        reset(gm)


def test_only_absolute_and_only_relative_tests(gm, world):
    """a list of one kind launches one kernel, and the rows are the same rows"""
    n_pkts = 300
    reset(gm)
    try:
        for pick in ([q for q in range(len(FIXED)) if q not in world.relative], [q for q in world.relative if q < len(FIXED)]):
            rows = world.rows[False][pick, :n_pkts]
            _not_trivial(rows)
            _setup(gm, world.payloads[:n_pkts], [world.tests[q] for q in pick])
            res = _check(gm, rows)
            assert res["timing"].launches == gm.scan_packets()["timing"].launches
    finally:
        reset(gm)


def test_windows_on_the_anchor(gm, world):
    """windows are pass state: the relative tests follow the anchor's window, the absolute ones do not care"""
    n_pkts = 700
    payloads = world.payloads[:n_pkts]
    windows = [(0, 6), (3, 40), (0, None)]
    tests = world.tests[:len(FIXED)]
    rows = BM.bytetest_rows(payloads, PATS, tests, windows, NOCASE, False)
    base = world.rows[False][:len(FIXED), :n_pkts]
    assert rows[1].any() and rows[1].sum() < base[1].sum() and not rows[1, 10]          # payload 10: its serving match is outside [0, 6]
    absolute = [q for q in range(len(FIXED)) if q not in world.relative]
    assert np.array_equal(rows[absolute], base[absolute])
    reset(gm)
    try:
        _setup(gm, payloads, tests)
        gm.set_windows(windows)
        _check(gm, rows)
        gm.set_windows([])
        _check(gm, base)
    finally:
        reset(gm)


def test_last_slot_of_a_borrowed_arena(gm):
    """The arena ends with its last slot, and the last payload's field ends on the slot's last byte: nothing behind it may be read.  Parity
    with the model; a read past the arena is the device's to report."""
    pay = [bytes(range(1, 32)), b"\x05" * 5, bytes(range(0x41, 0x61))]
    ln = np.array([len(t) for t in pay], dtype=np.uint32)
    off = np.array([0, 32, 48], dtype=np.uint64)
    arena = np.frombuffer(pay[0] + b"\xCC" + pay[1] + b"\xCC" * 11 + pay[2], dtype=np.uint8).copy()
    assert len(arena) == 80 and int(off[2]) + int(ln[2]) == 80
    tests = [bt(4, EQ, 0x5D5E5F60, 28), bt(1, EQ, 0x60, 31), bt(2, EQ, 0x605F, 30, little=True), bt(3, GE, 0, 29), bt(4, GE, 0, 29),
             bt(2, EQ, 0x5F60, 2, anchor=0), bt(1, GE, 0, 3, anchor=0), bt(4, EQ, 0x1C1D1E1F, 27), bt(4, GE, 0, 1), bt(1, EQ, 5, 4),
             bt(1, GE, 0, 4, anchor=0), bt(2, GE, 0, 3, anchor=0)]          # one byte past the last slot's end: never true
    pats = [bytes([0x5B, 0x5C])]
    rows = BM.bytetest_rows(pay, pats, tests)
    # payload 2 ends on the arena's last byte: the fields that end there hold, the ones a byte longer or further do not
    assert rows[:, 2].tolist() == [True, True, True, True, False, True, True, False, True, False, False, False]
    assert rows[:, 0].tolist() == [False] * 7 + [True, True, True, False, False] and rows[:, 1].tolist() == [False] * 8 + [True, True, False, False]
    keep = (torch.from_numpy(arena).cuda(), torch.from_numpy(off.astype(np.int64)).cuda(), torch.from_numpy(ln.astype(np.int32)).cuda())
    torch.cuda.synchronize()
    reset(gm)
    try:
        gm.set_option(OPT_REPACK, 0)
        for whole in (0, 1):
            gm.set_option(OPT_WHOLE_PAYLOAD, whole)
            gm.set_patterns(pats)
            gm.attach_arena(*keep)
            gm.set_bytetests(tests)
            _check(gm, rows)
    finally:
        reset(gm)
    del keep


# ------------------------------------------------------------------------------------------------
# 2. as rule terms: scan_rules, the alert list, the flows
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("whole", [False, True])
def test_byte_tests_as_rule_terms(gm, world, oracle, whole):
    n_pkts, n_bt = 1500, len(FIXED)
    payloads = world.payloads[:n_pkts]
    brows = world.rows[whole][:n_bt, :n_pkts]
    meta = meta_of_flows(np.arange(n_pkts) // 6 % 97)
    heads = [HM.header(sport=(1000, 1003)), HM.header(length=(16, 40))]
    lens = [len(t) for t in payloads]
    hrows = HM.header_rows(meta, lens, heads)
    relations = [(0, 1, None, None)]
    st = MM.starts(payloads, PATS, None, NOCASE, whole)
    mat = np.concatenate([MM.hits(st, len(PATS)), MM.relation_rows(st, PATS, relations), hrows, brows])
    np_, b0 = len(PATS), len(PATS) + 1 + 2
    h0 = np_ + 1
    rules = [([0, b0 + 1], []),                       # LEN: with a field above 0x0800 behind it
             ([b0 + 24], [b0 + 27]),                  # 1 .. 15 bytes of text: isdataat(0) and not isdataat(15)
             ([1], [b0 + 3, b0 + 31]),                # a negated relative test, and one that is never true
             ([h0 + 0, b0 + 32], [0]),                # a header term, the QR bit, no LEN:
             ([], [b0 + 24]),                         # a negated test alone: no byte of text at all -- the tail bits must stay 0
             ([b0 + 4, h0 + 1], [b0 + 20]),
             ([np_ + 0, b0 + 9], []),                 # a relation and a relative test
             ([b0 + 37, b0 + 38, b0 + 8, b0 + 10, b0 + 12], [b0 + 14])]
    want = MM.rule_rows(mat, rules)
    assert want.any(axis=1).all() and 0 < want.sum() < want.size
    counts = MM.oracle_counts(oracle, payloads, PATS, NOCASE, whole)
    reset(gm)
    try:
        gm.set_option(OPT_WHOLE_PAYLOAD, int(whole))
        gm.set_patterns(PATS, nocase=NOCASE)
        load(gm, payloads)
        gm.set_meta(meta)
        gm.set_relations(relations)
        gm.set_headers(heads)
        gm.set_bytetests(world.tests[:n_bt])
        assert [gm.rel(0), gm.hdr(0), gm.btest(0), gm.btest(n_bt - 1)] == [np_, h0, b0, b0 + n_bt - 1]
        with pytest.raises(ValueError):
            gm.btest(n_bt)
        gm.set_rules(rules)
        res = gm.scan_rules(hits=True)
        bad = np.argwhere(res["hits"] != want)
        assert bad.size == 0, [(int(r), int(k), bool(want[r, k])) for r, k in bad[:8]]
        assert res["rule_pkt_counts"].tolist() == want.sum(axis=1).tolist()
        assert res["any"].tolist() == want.any(axis=0).tolist()
        assert res["counts"].tolist() == counts
        # relation, header, two byte-test kernels and the rules kernel in the reduce's place
        assert res["timing"].launches == gm.scan_packets()["timing"].launches - 1 + 5
        # the rules family is how byte-test hits reach the alert list ...
        al = gm.scan_alerts("rules")
        assert [(int(a["packet"]), int(a["index"])) for a in al["alerts"]] == sorted((int(k), int(r)) for r, k in np.argwhere(want))
        assert al["n_found"] == int(want.sum()) and al["n_packets"] == int(want.any(axis=0).sum())
        # ... and the flows: under flow scope every term row is folded, the byte tests' among them
        gm.build_flows()
        fo = FM.flow_of_np(meta)
        want_f = FM.flow_rules(mat, fo, rules)
        assert 0 < want_f.sum() < want_f.size
        check_fold(gm, "rules", "flow", want_f, counts)
        check_fold(gm, "rules", "packet", FM.fold(want, fo), counts)
        # under a profile both kernels are recorded: two entries more than without byte tests
        gm.profile_begin(64)
        gm.scan_rules()
        with_b = len(gm.profile_end(64))
        gm.set_bytetests([])
        gm.set_rules([([0], [1])])
        gm.profile_begin(64)
        gm.scan_rules()
        assert with_b == len(gm.profile_end(64)) + 2
        # the tests' own rows, behind relations and headers
        gm.set_bytetests(world.tests[:n_bt])
        _check(gm, brows, counts)
    finally:
        reset(gm)


def test_alerts_have_no_byte_test_family(gm, world):
    reset(gm)
    _setup(gm, world.payloads[:64], world.tests[:3])
    found = _lib.C.c_uint64()
    for family in (4, 5):
        assert gm._g.kmpgpu_scan_alerts(gm._ctx, family, 10, _lib.C.byref(found), None, None, None, None) == EINVAL


# ------------------------------------------------------------------------------------------------
# 3. state
# ------------------------------------------------------------------------------------------------
def test_set_calls_drop_and_keep(gm, world):
    n = 200
    payloads, tests = world.payloads[:n], world.tests
    rows = world.rows[False][:, :n]
    meta = meta_of_flows(np.arange(n) % 5)
    reset(gm)
    gm.set_patterns(PATS, nocase=NOCASE)
    load(gm, payloads)
    gm.set_meta(meta)
    gm.set_rules([([0], [1])])
    before = gm.scan_rules(hits=True)
    # every successful kmpgpu_set_bytetests drops the rules
    gm.set_bytetests(tests[:6])
    with raises(ESTATE, "no rules set"):
        gm.scan_rules()
    gm.set_rules([([gm.btest(0)], [gm.btest(4)]), ([gm.btest(1)], [])])
    assert gm.scan_rules()["timing"].launches == before["timing"].launches + 2
    # kmpgpu_set_relations / _set_chains / _set_headers keep the byte tests (they name patterns, not rows) and drop the rules
    for setter, arg in ((gm.set_relations, [(0, 1, None, None)]), (gm.set_chains, [(0, (1, None, None))]), (gm.set_headers, [HM.header()])):
        gm.set_rules([([0], [])])
        setter(arg)
        with raises(ESTATE, "no rules set"):
            gm.scan_rules()
        _check(gm, rows[:6])
    assert gm.btest(0) == len(PATS) + 3
    gm.set_rules([([gm.btest(1)], []), ([gm.hdr(0)], [gm.btest(1)])])
    got = gm.scan_rules(hits=True)["hits"]
    assert np.array_equal(got[0], rows[1]) and np.array_equal(got[1], ~rows[1])
    # errors keep the earlier state: tests and rules
    bad = [dict(tests[0], nbytes=0), dict(tests[0], nbytes=5), dict(tests[0], op=6), dict(tests[0], flags=4), dict(tests[0], offset=-1),
           dict(tests[1], anchor=len(PATS))]
    for b in bad:
        with raises(EINVAL, "test 1"):
            gm.set_bytetests([tests[0], b])
    arr = np.zeros(2, dtype=BYTETEST_DTYPE)
    arr["nbytes"], arr["mask"] = 1, U32
    arr["reserved"][1] = 1
    with raises(EINVAL, "test 1: reserved is 1"):
        gm.set_bytetests(arr)
    arr["reserved"][1], arr["anchor"][1] = 0, 1           # an absolute test that names an anchor
    with raises(EINVAL, "test 1 is absolute and names anchor 1"):
        gm.set_bytetests(arr)
    assert gm._g.kmpgpu_set_bytetests(gm._ctx, None, 3) == EINVAL
    got = gm.scan_rules(hits=True)["hits"]
    assert np.array_equal(got[0], rows[1]) and np.array_equal(got[1], ~rows[1])
    _check(gm, rows[:6])
    # a BYTETEST_DTYPE array is taken as it is
    arr["anchor"][1] = 0
    arr["value"], arr["op"] = 0x41, GE
    gm.set_bytetests(arr)
    _check(gm, BM.bytetest_rows(payloads, PATS, [bt(1, GE, 0x41, 0)] * 2))
    # n_bt == 0 clears: the rules go, the rows are no terms any more, and with everything else cleared scan_rules is what it was
    gm.set_relations([])
    gm.set_chains([])
    gm.set_headers([])
    gm.set_bytetests(tests[:6])
    gm.set_rules([([gm.btest(5)], [])])
    gm.set_bytetests([])
    with raises(ESTATE, "no rules set"):
        gm.scan_rules()
    with raises(ESTATE, "no byte tests set"):
        gm.scan_bytetests()
    with raises(EINVAL, "names row 3"):
        gm.set_rules([([3], [])])
    gm.set_rules([([0], [1])])
    after = gm.scan_rules(hits=True)
    for key in ("hits", "rule_pkt_counts", "any", "counts"):
        assert np.array_equal(after[key], before[key]), key
    assert after["timing"].launches == before["timing"].launches
    # kmpgpu_set_patterns drops the byte tests with everything else
    gm.set_bytetests(tests[:6])
    gm.set_patterns(PATS, nocase=NOCASE)
    with raises(ESTATE, "no byte tests set"):
        gm.scan_bytetests()
    assert len(gm.bytetests) == 0
    # no patterns: ESTATE from both calls
    with GpuMatcher(0) as m:
        with raises(ESTATE, "no patterns set"):
            m.set_bytetests(tests[:1])
        with raises(ESTATE, "no patterns set"):
            m.scan_bytetests()


def test_no_payloads_and_no_outputs(gm, world):
    reset(gm)
    gm.set_patterns(PATS, nocase=NOCASE)
    gm.load_arena(HostArena.from_payloads([]))
    gm.set_bytetests(world.tests[:3])
    res = gm.scan_bytetests(hits=True)
    assert res["bt_pkt_counts"].tolist() == [0, 0, 0] and res["hits"].shape == (3, 0) and res["timing"].launches == 0
    gm.set_rules([([gm.btest(1)], [])])
    assert gm.scan_rules()["rule_pkt_counts"].tolist() == [0]
    # every output NULL: the pass runs and says nothing
    load(gm, world.payloads[:100])
    _lib.gpu_check(gm._g.kmpgpu_scan_bytetests(gm._ctx, None, None, None, None, None), "kmpgpu_scan_bytetests")
    assert gm._g.kmpgpu_scan_bytetests(None, None, None, None, None, None) == EINVAL
    _check(gm, world.rows[False][:3, :100])


def test_nothing_changes_without_byte_tests(gm, world):
    """with none set, scan_rules, scan_headers and scan_packets return what they return on a context that never had any"""
    n = 600
    payloads = world.payloads[:n]
    meta = meta_of_flows(np.arange(n) % 9)
    heads = [HM.header(sport=(1000, 1003)), HM.header(length=(16, 40))]

    def snapshot(m):
        m.set_relations([(0, 1, None, None)])
        m.set_headers(heads)
        m.set_rules([([0, m.hdr(1)], [1]), ([m.rel(0)], [m.hdr(0)])])
        out = []
        for res in (m.scan_rules(hits=True), m.scan_headers(hits=True), m.scan_packets(hits=True)):
            out.append((res["hits"].tobytes(), res["any"].tobytes(), res["counts"].tobytes(), res["timing"].launches,
                        [v.tobytes() for k, v in sorted(res.items()) if k.endswith("pkt_counts")]))
        return out

    reset(gm)
    with GpuMatcher(0) as fresh:
        for m in (gm, fresh):
            m.set_patterns(PATS, nocase=NOCASE)
            load(m, payloads)
            m.set_meta(meta)
        want = snapshot(fresh)
        gm.set_bytetests(world.tests[:40])
        gm.scan_bytetests()
        gm.set_rules([([gm.btest(0)], [])])
        gm.scan_rules()
        gm.set_bytetests([])
        assert snapshot(gm) == want


# ------------------------------------------------------------------------------------------------
# 4. the command line: KMPGPU_BYTETESTS_FILE
# ------------------------------------------------------------------------------------------------
def test_cli_byte_tests_file(tokens, tmp_path):
    pay, meta = HM.capture(HM.pcap_frames(os.path.join(DATA, "udp_1000.pcap")), "udp")
    n = len(tokens)
    hits = MM.hits(MM.starts(pay, tokens), n)
    busy = [int(i) for i in np.argsort(-hits.sum(axis=1))[:2]]
    tests = [bt(1, GE, 0x41, 0), bt(2, NE, 0, 2, mask=0x8000), BM.isdataat(100), bt(2, LT, 0x3000, 0, anchor=busy[0], little=True),
             bt(4, GT, 0x40000000, 4, mask=0x7F7F7F7F)]
    bf = tmp_path / "bytetests.txt"
    bf.write_text("# nbytes op value offset [after i] [little] [mask m]\n"
                  "1 >= 0x41 0\n"
                  "2 & 0x8000 2\n\n"
                  "1 >= 0 100\n"
                  f"2 < 0x3000 0 after {busy[0]} little\n"
                  "4 > 1073741824 4 mask 0x7f7f7f7f\n")
    brows = BM.bytetest_rows(pay, tokens, tests)
    assert all(0 < r.sum() < len(pay) for r in brows), brows.sum(axis=1).tolist()
    rules = [([busy[0], n + 0], []), ([busy[1]], [n + 1]), ([n + 3], []), ([], [n + 0, n + 1]), ([n + 4], [n + 3]), ([n + 1], [n + 2])]
    want = MM.rule_rows(np.concatenate([hits, brows]), rules)
    assert want.any(axis=1).all() and 0 < want.sum() < want.size

    def term(i):
        return str(i) if i < n else f"b{i - n}"

    rf = tmp_path / "rules.txt"
    rf.write_text("".join(" ".join([term(i) for i in pos] + ["!" + term(i) for i in neg]) + "\n" for pos, neg in rules))
    with open(os.path.join(GOLDEN, "stdout_udp_1000_udp.txt")) as f:
        golden = f.read()
    al = tmp_path / "alerts.csv"
    r = run_cli("serial", env_extra={"KMPGPU_BYTETESTS_FILE": str(bf), "KMPGPU_RULES_FILE": str(rf), "KMPGPU_ALERTS_FILE": str(al)})
    assert r.returncode == 0, r.stderr
    assert strip_elapsed(r.stdout) == golden
    got = [tuple(int(x) for x in line.split(",")) for line in al.read_text().splitlines()]
    assert got == sorted((int(k), int(r_)) for r_, k in np.argwhere(want))
