"""Regex rows on the GPU (kmpgpu_set_regexes / kmpgpu_scan_regexes, include/kmpgpu.h) against tests/regex_model.py, exactly: Python's re on
bytes and the gate, held to hand-written verdicts by tests/test_regex_model.py.

One synthetic capture is shared.  Its bytes come from a small alphabet (newlines, digits, blanks, both cases; 0x00 at chosen and at random
places), so that an expression splits the payloads; every test asserts on the model's rows that none under test is trivially empty or
full -- apart from the ones named as such -- before it looks at the device's.
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
import regex_model as RM
from regex_model import rx
from test_regex_model import HAND
from multithreading_string_matching_amd import _lib
from multithreading_string_matching_amd._lib import KmpGpuError
from multithreading_string_matching_amd.host import HostArena
from multithreading_string_matching_amd.matcher import OPT_FUSED, OPT_KERNEL, OPT_REPACK, OPT_WHOLE_PAYLOAD, GpuMatcher

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -2, -3
T = _lib.RX_TILE              # expressions the kernel stages at a time
ONES = 0xFFFFFFFFFFFFFFFF
N_MAX = 4097
N_PKTS = [1, 63, 64, 65, 255, 256, 257, N_MAX]
N_RX = [1, T - 1, T, T + 1, 3 * T + 1]
LENS = [0, 1, 3, 15, 16, 17, 32, 40, 1500]
ALPHA = b"\n\n  0189aAbBxX=:/"
PATS = [b"GET", b"host", b"key=", b"ZZZZQ"]            # a plain one, a nocase one, one that gets a window, one that no payload holds
NOCASE = [False, True, False, False]
WINDOWS = [(0, None), (0, None), (2, 20), (0, None)]

# the texts of the hand cases of tests/test_regex_model.py, planted as the first payloads, then the position budget's
PLANTED = [b"ab7"] + [t for _, _, t, _, _ in HAND] + [b"bbb" + b"a" * 63 + b"bbbb", b"bbb" + b"a" * 62 + b"bbbb", b"q" * 62 + b"x", b"q" * 63 + b"x",
                                           b"0123456789" * 150, b"0123456789" * 149 + b"012345678\n", b"=" + b"a" * 20 + b":", b"=" + b"a" * 21 + b":"]


def raises(code, text):
    return pytest.raises(KmpGpuError, match=rf"\({code}\).*{text}")


def _capture(n, seed=11):
    rng = np.random.default_rng(seed)
    lens = rng.choice(LENS, n)
    alpha = np.frombuffer(ALPHA, dtype=np.uint8)
    out = []
    for k in range(n):
        L = int(lens[k])
        b = bytearray(rng.choice(alpha, L).tobytes())
        if k % 4 != 1:                                                 # every fourth payload keeps no 0x00
            for z in np.flatnonzero(rng.integers(0, 40, L) == 0):      # 0x00 at random places ...
                b[int(z)] = 0
            if L >= 17 and k % 3 == 0:                                 # ... and at bytes 13 and 16 of every third
                b[13 if k % 2 else 16] = 0
        if L >= 15:                                                    # the gates' patterns
            for _ in range(1 + L // 300):
                word = [b"GET", b"host", b"HoSt", b"key=", b"key="][int(rng.integers(5))]
                at = int(rng.integers(0, L - len(word)))
                b[at:at + len(word)] = word
        out.append(bytes(b))
    out[:len(PLANTED)] = PLANTED[:n]
    if n == N_MAX:                                                     # the arena's last payload fills its slot: no padding byte to stop on
        out[-1] = b"a=1 " * 7 + b"GET7"
        assert len(out[-1]) % 16 == 0
    return out


# gated and ungated expressions take turns; ALL, EMPTY and WHOLE_ONLY below name the rows that are full or empty by design
EXPRS = [
    b"[0-9]$",                                             # a match that ends exactly at E_k: a 0x00 right behind it, or L_k
    rx(b"[aA]=", gate=0),
    rx(b"x[^a]", nocase=True),                             # nocase against [^a]
    rx(b"a.b", gate=1),                                    # the dot against \n ...
    rx(b"a.b", dotall=True),                               # ... with dotall
    rx(b"^\\s*$", gate=3),                                 # a gate nobody holds: empty
    b"^\\s*$",                                             # $ on the empty payload
    rx(b"\\d{3,}", gate=2),
    b"x*",                                                 # matches the empty string: full
    rx(b"^.{14}[aA]", dotall=True, gate=0),                # matches that end at bytes 15, 16, 17: across the 16-byte load
    rx(b"^.{15}[aA]", dotall=True),
    rx(b"^.{16}[aA]", dotall=True, gate=1),
    b"a{63}",                                              # the position budget: accept bit 63
    rx(b".{0,62}x", gate=0),
    b"^\\d+$",                                             # ^...$ on a 1500-byte payload of one class
    rx(b"=a?b", gate=2),                                   # runs of 1, 20 and 62 optional positions
    b"=a{0,20}:",
    rx(b"^[^\\n]{0,62}$", gate=1),
    b"a\\x00",                                             # needs a 0x00 as a text byte: whole payloads only
    rx(b"[ \\n]{2}\\w+=", gate=0),
    b"\\D\\d\\D",
    rx(b"^.{0,62}x$", dotall=True),
    b"[^\\x00-\\x2f]{6}",
    rx(b"HOST[:= ]", nocase=True, gate=1),
    b"key=\\S{2,}\\s",
]
ALL, EMPTY, WHOLE_ONLY = {8}, {5}, {18}
assert len(EXPRS) == 3 * T + 1 and [isinstance(e, tuple) and "gate" in e[1] for e in EXPRS[:20]] == [False, True] * 10


class World:
    def __init__(self):
        self.payloads = _capture(N_MAX)
        self.hits = {w: MM.hits(MM.starts(self.payloads, PATS, None, NOCASE, w), len(PATS)) for w in (False, True)}
        self.rows = {w: RM.regex_rows(self.payloads, EXPRS, w, self.hits[w]) for w in (False, True)}


@pytest.fixture(scope="module")
def world():
    w = World()
    n = len(w.payloads)
    assert not w.hits[True][3].any() and all(0 < w.hits[x][i].sum() < n for x in (False, True) for i in range(3))
    for whole in (False, True):
        rows = w.rows[whole]
        for q in range(len(EXPRS)):
            if q in EMPTY or (not whole and q in WHOLE_ONLY):
                assert not rows[q].any(), (q, whole)
            elif q in ALL:
                assert rows[q].all(), (q, whole)
            else:
                assert 0 < rows[q].sum() < n, (q, whole, EXPRS[q], int(rows[q].sum()))
    # the planted payloads, bit by bit
    s, wh = w.rows[False], w.rows[True]
    at = len(HAND) + 1
    assert s[12, at] and not s[12, at + 1] and wh[12, at]                           # 63 a's and 62
    assert s[21, at + 2] and not s[21, at + 3] and s[13, at + 2] == w.hits[False][0, at + 2]     # 62 bytes and an x, 63 and an x
    assert s[14, at + 4] and not s[14, at + 5] and len(w.payloads[at + 4]) == 1500    # 1500 digits; a newline at the end
    assert s[16, at + 6] and not s[16, at + 7]                                      # 20 optional positions taken, 21 needed
    empty = [k for k, t in enumerate(w.payloads) if not t]
    assert empty and s[6, empty].all() and s[8, empty].all() and not s[0, empty].any()
    # matches that end exactly at E_k with a 0x00 right behind them, and at L_k
    ends = [k for k, t in enumerate(w.payloads) if 0 < t.find(b"\0") < len(t) and t[t.find(b"\0") - 1:t.find(b"\0")].isdigit()]
    assert len(ends) > 20 and s[0, ends].all()
    assert any(wh[0, k] and b"\0" not in w.payloads[k] for k in range(n))
    return w


def _not_trivial(rows):
    if rows.size == 1:
        assert rows.sum() == 1
    else:
        assert 0 < rows.sum() < rows.size


def _check(m, rows, counts=None):
    res = m.scan_regexes(hits=True)
    bad = np.argwhere(res["hits"] != rows)
    assert bad.size == 0, [(int(q), int(k), bool(rows[q, k]), m.regexes[int(q)]) for q, k in bad[:6]]
    assert res["rx_pkt_counts"].tolist() == rows.sum(axis=1).tolist()
    assert res["any"].tolist() == rows.any(axis=0).tolist()
    if counts is not None:
        assert res["counts"].tolist() == list(counts)
    return res


def _setup(m, payloads, exprs, whole=False):
    m.set_option(OPT_WHOLE_PAYLOAD, int(whole))
    m.set_patterns(PATS, nocase=NOCASE)
    load(m, payloads)
    m.set_regexes(exprs)


# ------------------------------------------------------------------------------------------------
# 1. rows against the model
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("whole", [False, True])
@pytest.mark.parametrize("n_pkts", N_PKTS)
def test_rows_against_the_model(gm, world, n_pkts, whole):
    """the word edges and the block's four-word edge, times the tile loop's edges"""
    reset(gm)
    try:
        gm.set_option(OPT_WHOLE_PAYLOAD, int(whole))
        gm.set_patterns(PATS, nocase=NOCASE)
        load(gm, world.payloads[:n_pkts])
        plain = gm.scan_packets()
        for n_rx in N_RX:
            rows = world.rows[whole][:n_rx, :n_pkts]
            _not_trivial(rows)
            gm.set_regexes(EXPRS[:n_rx])
            res = _check(gm, rows, plain["counts"].tolist())
            # the marking pass, and one kernel in the reduce's place
            assert res["timing"].launches == plain["timing"].launches
            # the raw words: the bits at n_pkts and above are 0, also for x*
            W = (n_pkts + 63) // 64
            hit_w, any_w = np.full((n_rx, W), ONES, dtype=np.uint64), np.full(W, ONES, dtype=np.uint64)
            _lib.gpu_check(gm._g.kmpgpu_scan_regexes(gm._ctx, None, any_w.ctypes.data, hit_w.ctypes.data, None, None), "kmpgpu_scan_regexes")
            assert np.array_equal(hit_w, MM.words(rows)) and np.array_equal(any_w, MM.words(rows.any(axis=0)))
    finally:
        reset(gm)


@pytest.mark.parametrize("name,kernel,fused", KERNELS)
@pytest.mark.parametrize("whole", [False, True])
def test_every_streaming_kernel_selection(gm, world, oracle, whole, name, kernel, fused):
    n_pkts = 1000
    rows = world.rows[whole][:, :n_pkts]
    _not_trivial(rows)
    counts = MM.oracle_counts(oracle, world.payloads[:n_pkts], PATS, NOCASE, whole)
    reset(gm)
    try:
        gm.set_option(OPT_KERNEL, kernel)
        gm.set_option(OPT_FUSED, fused)
        _setup(gm, world.payloads[:n_pkts], EXPRS, whole)
        _check(gm, rows, counts)
    finally:
        reset(gm)


def test_both_text_end_rules_on_one_context(gm, world):
    """KMPGPU_OPT_WHOLE_PAYLOAD is pass state: switched between two passes with nothing set again"""
    n_pkts = 2000
    reset(gm)
    try:
        _setup(gm, world.payloads[:n_pkts], EXPRS, False)
        assert (world.rows[False][:, :n_pkts] != world.rows[True][:, :n_pkts]).any(axis=1).sum() > len(EXPRS) // 2
        for whole in (False, True, False):
            gm.set_option(OPT_WHOLE_PAYLOAD, int(whole))
            _check(gm, world.rows[whole][:, :n_pkts])
    finally:
        reset(gm)


def test_gates(gm, world):
    """a gated row is the model's ungated row and-ed with the gate pattern's scan_packets row -- the device's own too: a plain pattern, a
    nocase one, one under a window, and one that no payload holds"""
    n_pkts = 3000
    payloads = world.payloads[:n_pkts]
    body = [b"[aA]=", b"\\d{3,}", b"x*", b"^[^\\n]{0,62}$"]
    exprs = [rx(e, gate=g) for g in range(4) for e in body] + body
    reset(gm)
    try:
        for windows in (None, WINDOWS):
            hits = MM.hits(MM.starts(payloads, PATS, windows, NOCASE, False), len(PATS))
            rows = RM.regex_rows(payloads, exprs, False, hits)
            free = rows[16:]
            for g in range(4):
                assert np.array_equal(rows[4 * g:4 * g + 4], free & hits[g])
                assert (not rows[4 * g:4 * g + 4].any()) if g == 3 else all(0 < r.sum() < f.sum() for r, f in zip(rows[4 * g:4 * g + 4], free))
            _setup(gm, payloads, exprs)
            if windows:
                gm.set_windows(windows)
            res = _check(gm, rows)
            dev = gm.scan_packets(hits=True)["hits"]
            assert np.array_equal(dev, hits)
            for g in range(4):
                assert np.array_equal(res["hits"][4 * g:4 * g + 4], res["hits"][16:] & dev[g])
        assert hits[2].sum() < world.hits[False][2, :n_pkts].sum()                  # the window took some of the gate's payloads away
    finally:
        reset(gm)


def test_last_slot_of_a_borrowed_arena(gm):
    """The arena ends with its last slot, and the last payload fills it to the last byte: there is no padding byte to stop on, and nothing
    behind the slot may be read.  Parity with the model; a read past the arena is the device's to report."""
    pay = [b"0123456789abcdef" * 2, b"ab\0cd", b"a=1 " * 7 + b"GET7", b"x" * 16]
    sizes = [32, 16, 32, 16]
    arena = np.frombuffer(b"".join(t + b"\xCC" * (s - len(t)) for t, s in zip(pay, sizes)), dtype=np.uint8).copy()
    off = np.array([0, 32, 48, 80], dtype=np.uint64)
    ln = np.array([len(t) for t in pay], dtype=np.uint32)
    assert len(arena) == 96 == int(off[3]) + int(ln[3])
    exprs = [b"[0-9]$", b"x{16}$", b"^x{17}", b"f$", b"\\xcc", b"T7$", rx(b"^.{31}7$", gate=0), b"cd", b"x{15}.$"]
    pats = [b"GET"]
    keep = (torch.from_numpy(arena).cuda(), torch.from_numpy(off.astype(np.int64)).cuda(), torch.from_numpy(ln.astype(np.int32)).cuda())
    torch.cuda.synchronize()
    reset(gm)
    try:
        gm.set_option(OPT_REPACK, 0)
        for whole in (False, True):
            hits = MM.hits(MM.starts(pay, pats, None, None, whole), 1)
            rows = RM.regex_rows(pay, exprs, whole, hits)
            assert rows[:, 3].tolist() == [False, True, False, False, False, False, False, False, True]
            assert rows[:, 2].tolist() == [True, False, False, False, False, True, True, False, False] and not rows[4].any()
            assert rows[7].tolist() == [True, whole, False, False]
            gm.set_option(OPT_WHOLE_PAYLOAD, int(whole))
            gm.set_patterns(pats)
            gm.attach_arena(*keep)
            gm.set_regexes(exprs)
            _check(gm, rows)
    finally:
        reset(gm)
    del keep


# ------------------------------------------------------------------------------------------------
# 2. as rule terms: scan_rules, the alert list, the flows, the selection
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("whole", [False, True])
def test_expressions_as_rule_terms(gm, world, oracle, whole):
    n_pkts = 1500
    payloads = world.payloads[:n_pkts]
    xrows = world.rows[whole][:, :n_pkts]
    meta = meta_of_flows(np.arange(n_pkts) // 6 % 97)
    heads = [HM.header(sport=(1000, 1003)), HM.header(length=(16, 40))]
    hrows = HM.header_rows(meta, [len(t) for t in payloads], heads)
    tests = [BM.bt(1, BM.GE, 0x41, 0), BM.isdataat(15)]
    st = MM.starts(payloads, PATS, None, NOCASE, whole)
    brows = BM.bytetest_rows(payloads, PATS, tests, None, NOCASE, whole, st)
    mat = np.concatenate([MM.hits(st, len(PATS)), hrows, brows, xrows])
    np_ = len(PATS)
    h0, b0, x0 = np_, np_ + 2, np_ + 4
    rules = [([0, x0 + 1], []),                       # GET with a= behind its gate
             ([x0 + 0], [x0 + 20]),                   # ends with a digit, no digit between two non-digits
             ([1], [x0 + 3, x0 + 5]),                 # a negated gated expression, and one that is never true
             ([h0 + 0, x0 + 2], [0]),                 # a header term, an expression, no GET
             ([], [x0 + 6, x0 + 0]),                  # negated expressions alone -- the tail bits must stay 0
             ([b0 + 0, x0 + 4], [b0 + 1]),            # a byte test on either side
             ([x0 + 8, x0 + 16], []),                 # the full row changes nothing
             ([x0 + 24, 2], [x0 + 19])]
    want = MM.rule_rows(mat, rules)
    assert want.any(axis=1).all() and 0 < want.sum() < want.size
    counts = MM.oracle_counts(oracle, payloads, PATS, NOCASE, whole)
    reset(gm)
    try:
        gm.set_option(OPT_WHOLE_PAYLOAD, int(whole))
        gm.set_patterns(PATS, nocase=NOCASE)
        load(gm, payloads)
        gm.set_meta(meta)
        gm.set_headers(heads)
        gm.set_bytetests(tests)
        gm.set_regexes(EXPRS)
        assert [gm.hdr(0), gm.btest(0), gm.regex(0), gm.regex(len(EXPRS) - 1)] == [h0, b0, x0, x0 + len(EXPRS) - 1]
        with pytest.raises(ValueError):
            gm.regex(len(EXPRS))
        gm.set_rules(rules)
        res = gm.scan_rules(hits=True)
        bad = np.argwhere(res["hits"] != want)
        assert bad.size == 0, [(int(r), int(k), bool(want[r, k])) for r, k in bad[:8]]
        assert res["rule_pkt_counts"].tolist() == want.sum(axis=1).tolist()
        assert res["any"].tolist() == want.any(axis=0).tolist()
        assert res["counts"].tolist() == counts
        # header, byte-test, regex and rules kernel in the reduce's place
        assert res["timing"].launches == gm.scan_packets()["timing"].launches - 1 + 4
        # the rules family is how the expressions' hits reach the alert list ...
        al = gm.scan_alerts("rules")
        assert [(int(a["packet"]), int(a["index"])) for a in al["alerts"]] == sorted((int(k), int(r)) for r, k in np.argwhere(want))
        assert al["n_found"] == int(want.sum()) and al["n_packets"] == int(want.any(axis=0).sum())
        # ... the selection ...
        with GpuMatcher(0) as dst:
            idx = dst.load_selected(gm, res["any"])
            assert idx.tolist() == np.flatnonzero(want.any(axis=0)).tolist()
        # ... and the flows: under flow scope every term row is folded, the expressions' among them
        gm.build_flows()
        fo = FM.flow_of_np(meta)
        want_f = FM.flow_rules(mat, fo, rules)
        assert 0 < want_f.sum() < want_f.size
        check_fold(gm, "rules", "flow", want_f, counts)
        check_fold(gm, "rules", "packet", FM.fold(want, fo), counts)
        # under a profile the regex kernel is one recorded launch
        gm.profile_begin(64)
        gm.scan_rules()
        with_x = len(gm.profile_end(64))
        gm.set_regexes([])
        gm.set_rules([([0], [1])])
        gm.profile_begin(64)
        gm.scan_rules()
        assert with_x == len(gm.profile_end(64)) + 1
        # the expressions' own rows, behind headers and byte tests
        gm.set_regexes(EXPRS)
        _check(gm, xrows, counts)
    finally:
        reset(gm)


def test_alerts_have_no_regex_family(gm, world):
    reset(gm)
    _setup(gm, world.payloads[:64], EXPRS[:3])
    found = _lib.C.c_uint64()
    for family in (4, 5, 6):
        assert gm._g.kmpgpu_scan_alerts(gm._ctx, family, 10, _lib.C.byref(found), None, None, None, None) == EINVAL


# ------------------------------------------------------------------------------------------------
# 3. state
# ------------------------------------------------------------------------------------------------
def test_set_calls_drop_and_keep(gm, world):
    n = 200
    payloads = world.payloads[:n]
    rows = world.rows[False][:, :n]
    meta = meta_of_flows(np.arange(n) % 5)
    reset(gm)
    gm.set_patterns(PATS, nocase=NOCASE)
    load(gm, payloads)
    gm.set_meta(meta)
    gm.set_rules([([0], [1])])
    before = gm.scan_rules(hits=True)
    # every successful kmpgpu_set_regexes drops the rules
    gm.set_regexes(EXPRS[:6])
    with raises(ESTATE, "no rules set"):
        gm.scan_rules()
    gm.set_rules([([gm.regex(0)], [gm.regex(4)]), ([gm.regex(1)], [])])
    assert gm.scan_rules()["timing"].launches == before["timing"].launches + 1
    # the other setters keep the expressions (they name patterns, not rows) and drop the rules
    for setter, arg in ((gm.set_relations, [(0, 1, None, None)]), (gm.set_chains, [(0, (1, None, None))]), (gm.set_headers, [HM.header()]),
                        (gm.set_bytetests, [BM.isdataat(3)])):
        gm.set_rules([([0], [])])
        setter(arg)
        with raises(ESTATE, "no rules set"):
            gm.scan_rules()
        _check(gm, rows[:6])
    assert gm.regex(0) == len(PATS) + 4
    gm.set_rules([([gm.regex(1)], []), ([gm.hdr(0)], [gm.regex(1)])])
    got = gm.scan_rules(hits=True)["hits"]
    assert np.array_equal(got[0], rows[1]) and np.array_equal(got[1], ~rows[1])
    # errors keep the earlier state: expressions and rules
    for bad, what in ((b"a(b)", "expression 1: position 1: '\\(' is reserved"), (b"a**", "expression 1: position 2: a quantifier on a quantifier"),
                      (b"a{64}", "expression 1: position 0: more than 63 positions"), (b"", "expression 1: position 0: zero elements"),
                      (b"a\0b", "expression 1: position 1: a raw 0x00"), (rx(b"a", gate=len(PATS)), "expression 1: its gate names pattern 4 of 4")):
        with raises(EINVAL, what):
            gm.set_regexes([b"ok", bad])
    u32 = np.array([0, 8, 0, 1], dtype=np.uint32)
    ptrs = (_lib.C.c_char_p * 2)(b"a", b"b")
    lens = np.array([1, 1], dtype=np.uint32)
    assert gm._g.kmpgpu_set_regexes(gm._ctx, ptrs, lens.ctypes.data_as(_lib.u32p), u32[:2].ctypes.data_as(_lib.u32p), None, 2) == EINVAL      # flag 8
    assert b"unknown flag bits 0x8" in gm._g.kmpgpu_last_error()
    assert gm._g.kmpgpu_set_regexes(gm._ctx, ptrs, lens.ctypes.data_as(_lib.u32p), None, u32[2:].ctypes.data_as(_lib.u32p), 2) == EINVAL       # a gate, not gated
    assert b"expression 1 is not gated and names gate 1" in gm._g.kmpgpu_last_error()
    assert gm._g.kmpgpu_set_regexes(gm._ctx, None, None, None, None, 3) == EINVAL
    got = gm.scan_rules(hits=True)["hits"]
    assert np.array_equal(got[0], rows[1]) and np.array_equal(got[1], ~rows[1])
    _check(gm, rows[:6])
    # n_rx == 0 clears: the rules go, the rows are no terms any more, and with everything else cleared scan_rules is what it was
    gm.set_relations([])
    gm.set_chains([])
    gm.set_headers([])
    gm.set_bytetests([])
    gm.set_regexes(EXPRS[:6])
    gm.set_rules([([gm.regex(5)], [])])
    gm.set_regexes([])
    with raises(ESTATE, "no rules set"):
        gm.scan_rules()
    with raises(ESTATE, "no expressions set"):
        gm.scan_regexes()
    with raises(EINVAL, "names row 4"):
        gm.set_rules([([4], [])])
    gm.set_rules([([0], [1])])
    after = gm.scan_rules(hits=True)
    for key in ("hits", "rule_pkt_counts", "any", "counts"):
        assert np.array_equal(after[key], before[key]), key
    assert after["timing"].launches == before["timing"].launches
    # kmpgpu_set_patterns drops the expressions with everything else
    gm.set_regexes(EXPRS[:6])
    gm.set_patterns(PATS, nocase=NOCASE)
    with raises(ESTATE, "no expressions set"):
        gm.scan_regexes()
    assert len(gm.regexes) == 0
    # no patterns: ESTATE from both calls
    with GpuMatcher(0) as m:
        with raises(ESTATE, "no patterns set"):
            m.set_regexes([b"a"])
        with raises(ESTATE, "no patterns set"):
            m.scan_regexes()


def test_no_payloads_and_no_outputs(gm, world):
    reset(gm)
    gm.set_patterns(PATS, nocase=NOCASE)
    gm.load_arena(HostArena.from_payloads([]))
    gm.set_regexes(EXPRS[:3])
    res = gm.scan_regexes(hits=True)
    assert res["rx_pkt_counts"].tolist() == [0, 0, 0] and res["hits"].shape == (3, 0) and res["timing"].launches == 0
    gm.set_rules([([gm.regex(1)], [])])
    assert gm.scan_rules()["rule_pkt_counts"].tolist() == [0]
    # every output NULL: the pass runs and says nothing
    load(gm, world.payloads[:100])
    _lib.gpu_check(gm._g.kmpgpu_scan_regexes(gm._ctx, None, None, None, None, None), "kmpgpu_scan_regexes")
    assert gm._g.kmpgpu_scan_regexes(None, None, None, None, None, None) == EINVAL
    _check(gm, world.rows[False][:3, :100])


def test_nothing_changes_without_expressions(gm, world):
    """with none set, scan_rules, scan_bytetests, scan_headers and scan_packets return what they return on a context that never had any"""
    n = 600
    payloads = world.payloads[:n]
    meta = meta_of_flows(np.arange(n) % 9)
    heads = [HM.header(sport=(1000, 1003)), HM.header(length=(16, 40))]

    def snapshot(m):
        m.set_relations([(0, 1, None, None)])
        m.set_headers(heads)
        m.set_bytetests([BM.isdataat(15), BM.bt(1, BM.GE, 0x41, 0, anchor=0)])
        m.set_rules([([0, m.hdr(1)], [1]), ([m.rel(0)], [m.hdr(0)]), ([m.btest(0)], [m.btest(1)])])
        out = []
        for res in (m.scan_rules(hits=True), m.scan_bytetests(hits=True), m.scan_headers(hits=True), m.scan_packets(hits=True)):
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
        gm.set_regexes(EXPRS)
        gm.scan_regexes()
        gm.set_rules([([gm.regex(0)], [])])
        gm.scan_rules()
        gm.set_regexes([])
        assert snapshot(gm) == want


# ------------------------------------------------------------------------------------------------
# 4. the command line: KMPGPU_REGEX_FILE
# ------------------------------------------------------------------------------------------------
def _cli_case(tokens):
    pay, meta = HM.capture(HM.pcap_frames(os.path.join(DATA, "udp_1000.pcap")), "udp")
    n = len(tokens)
    hits = MM.hits(MM.starts(pay, tokens), n)
    busy = [int(i) for i in np.argsort(-hits.sum(axis=1))[:2]]
    exprs = [rx(b"[a-z]{6,}", nocase=True), b"^[\\x00-\\x1f]", rx(b"\\d{2,}[^0-9]", gate=busy[0]), rx(b"^.{40,}$", dotall=True), b"[a-z]+/[a-z]+"]
    text = ("# /EXPR/[i][s] [with <pattern index>]\n"
            "/[a-z]{6,}/i\n"
            "/^[\\x00-\\x1f]/\n\n"
            f"/\\d{{2,}}[^0-9]/ with {busy[0]}\n"
            "/^.{40,}$/s\n"
            "/[a-z]+/[a-z]+/\n")
    xrows = RM.regex_rows(pay, exprs, False, hits)
    rules = [([busy[0], n + 0], []), ([busy[1]], [n + 1]), ([n + 2], []), ([], [n + 0, n + 1]), ([n + 3], [n + 2]), ([n + 1], [n + 4])]
    return pay, hits, text, xrows, rules


def test_cli_expressions_file(tokens, tmp_path):
    pay, hits, text, xrows, rules = _cli_case(tokens)
    n = len(tokens)
    assert all(0 < r.sum() < len(pay) for r in xrows), xrows.sum(axis=1).tolist()
    want = MM.rule_rows(np.concatenate([hits, xrows]), rules)
    assert want.any(axis=1).all() and 0 < want.sum() < want.size
    xf = tmp_path / "regex.txt"
    xf.write_text(text)

    def term(i):
        return str(i) if i < n else f"x{i - n}"

    rf = tmp_path / "rules.txt"
    rf.write_text("".join(" ".join([term(i) for i in pos] + ["!" + term(i) for i in neg]) + "\n" for pos, neg in rules))
    with open(os.path.join(GOLDEN, "stdout_udp_1000_udp.txt")) as f:
        golden = f.read()
    al = tmp_path / "alerts.csv"
    r = run_cli("serial", env_extra={"KMPGPU_REGEX_FILE": str(xf), "KMPGPU_RULES_FILE": str(rf), "KMPGPU_ALERTS_FILE": str(al)})
    assert r.returncode == 0, r.stderr
    assert strip_elapsed(r.stdout) == golden
    got = [tuple(int(x) for x in line.split(",")) for line in al.read_text().splitlines()]
    assert got == sorted((int(k), int(r_)) for r_, k in np.argwhere(want))
    # an expression outside the dialect is refused when the shard is set up, with the library's message
    xf.write_text("/a(b)/\n")
    rf.write_text("x0\n")
    r = run_cli("serial", env_extra={"KMPGPU_REGEX_FILE": str(xf), "KMPGPU_RULES_FILE": str(rf), "KMPGPU_ALERTS_FILE": str(al)})
    assert r.returncode != 0 and "expression 0: position 1: '(' is reserved" in r.stderr, r.stderr
