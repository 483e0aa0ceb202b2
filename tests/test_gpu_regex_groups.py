"""Regex rows under KMPGPU_RX_GROUPS on the GPU -- groups and alternation, kmp_regex_groups.hip -- against tests/regex_model.py, exactly:
Python's re on bytes and the gate.  The capture, the patterns and the comparison are those of tests/test_gpu_regex.py; every test asserts on
the model's rows that none under test is trivially empty or full before it looks at the device's."""
import numpy as np
import pytest

from gpu_support import gm, load, reset  # noqa: F401  (gm: the context fixture)

import match_model as MM
import regex_model as RM
from test_gpu_regex import EINVAL, NOCASE, ONES, PATS, _capture, _check, _setup, raises
from multithreading_string_matching_amd import _lib
from multithreading_string_matching_amd.matcher import OPT_WHOLE_PAYLOAD

pytestmark = pytest.mark.gpu

T, TG = _lib.RX_TILE, _lib.RXG_TILE
N_MAX = 257


def g(expr, **opt):
    return (expr, dict(opt, groups=True))


def plain(e):
    """the expression as the model takes it: `groups` is the library's business alone"""
    expr, opt = (e, {}) if isinstance(e, bytes) else e
    return (expr, {k: v for k, v in opt.items() if k != "groups"})


# what the linear dialect refuses, each with a group or an alternation that matters on the capture of test_gpu_regex.py
GROUPED = [b"(GET|host|key=)[ =/:]", b"(a|b)(x|X)", b"^(\\d|[ab])+$", b"(0|1)(8|9)+(a|A)?=", b"(ab|ba){2}", b"(?:x[aA]|=:)", b"a9|B9|x=",
           b"((a|b)x)+\\d", b"(\\s|/)(a(b|B)|\\d{2,})", b"(x+|a)b$", b"(aA|[bB]x?){1,3}:"]
LINEAR = [b"[0-9]$", b"[aA]=", b"a.b", b"\\d{3,}", b"^\\s*$", b"\\D\\d\\D", b"key=\\S{2,}\\s", b"=a?b", b"x[^a]", b"[ \\n]{2}\\w+="]


def _mixed(n):
    """n expressions, flagged and unflagged taking turns, every other flagged one gated"""
    out = []
    for i in range(n):
        if i % 2 == 0:
            e = GROUPED[(i // 2) % len(GROUPED)]
            out.append(g(e, gate=(i // 4) % 3) if i % 4 == 2 else g(e))
        else:
            out.append(LINEAR[(i // 2) % len(LINEAR)])
    return out


class World:
    def __init__(self):
        self.payloads = _capture(N_MAX)
        self.hits = {w: MM.hits(MM.starts(self.payloads, PATS, None, NOCASE, w), len(PATS)) for w in (False, True)}

    def rows(self, exprs, whole=False, n=N_MAX):
        return RM.regex_rows(self.payloads[:n], [plain(e) for e in exprs], whole, self.hits[whole][:, :n])


@pytest.fixture(scope="module")
def world():
    w = World()
    for whole in (False, True):
        rows = w.rows(GROUPED + LINEAR, whole)
        assert all(0 < r.sum() < N_MAX for r in rows), rows.sum(axis=1).tolist()
    return w


def test_a_flagged_set_loads_and_matches(gm, world):
    """(on a library without the feature: KMPGPU_EINVAL, unknown flag bits 0x10)"""
    exprs = [g(e) for e in GROUPED]
    reset(gm)
    try:
        _setup(gm, world.payloads, exprs)
        assert all(f & _lib.RX_GROUPS for _, f, _ in gm.regexes)
        _check(gm, world.rows(exprs))
    finally:
        reset(gm)


@pytest.mark.parametrize("whole", [False, True])
def test_text_lengths_and_load_edges(gm, whole):
    """a match that starts or ends at each 16-byte edge, one that only exists across it, and a 0x00 inside a would-be match"""
    word = b"POST /"
    pay = []
    for L in (0, 1, 15, 16, 17, 31, 32, 33, 100):
        pay.append(b"x" * L)
        for s in list(range(8, 18)) + list(range(24, 34)) + [L - len(word)]:
            if 0 <= s and s + len(word) <= L:
                t = bytearray(b"x" * L)
                t[s:s + len(word)] = word
                pay.append(bytes(t))
                t[s + 2] = 0                                   # PO\0T /: no match under either rule, and the text ends here under the default
                pay.append(bytes(t))
                t[s:s + len(word)] = word
                if s + len(word) < L:
                    t[s + len(word)] = 0                       # a 0x00 right behind the match
                    pay.append(bytes(t))
    exprs = [g(b"(GET|POST) /"), g(b"(GET|POST) /$"), g(b"^(x|y)+$"), g(b"^(x{16}|y)(x|P)"), g(b"(x|\\x00)(POST|\\x00T) /(x|\\x00)", dotall=True),
             g(b"^(x{15}|x{31})(PO)"), b"POST /", g(b"(xP|xx)OST")]
    hits = MM.hits(MM.starts(pay, PATS, None, NOCASE, whole), len(PATS))
    rows = RM.regex_rows(pay, [plain(e) for e in exprs], whole, hits)
    assert all(0 < r.sum() < len(pay) for r in rows), rows.sum(axis=1).tolist()
    assert np.array_equal(rows[0], rows[6])
    reset(gm)
    try:
        _setup(gm, pay, exprs, whole)
        _check(gm, rows)
    finally:
        reset(gm)


@pytest.mark.parametrize("n_pkts", [1, 63, 64, 65, 257])
def test_mixed_sets_and_tile_edges(gm, world, n_pkts):
    reset(gm)
    try:
        gm.set_patterns(PATS, nocase=NOCASE)
        load(gm, world.payloads[:n_pkts])
        for n_rx in (1, TG, TG + 1, 2 * TG + 1, 2 * T + 3):
            exprs = _mixed(n_rx)
            rows = world.rows(exprs, False, n_pkts)
            if n_pkts > 1:
                assert 0 < rows.sum() < rows.size
            gm.set_regexes(exprs)
            _check(gm, rows)
            W = (n_pkts + 63) // 64
            hit_w, any_w = np.full((n_rx, W), ONES, dtype=np.uint64), np.full(W, ONES, dtype=np.uint64)
            _lib.gpu_check(gm._g.kmpgpu_scan_regexes(gm._ctx, None, any_w.ctypes.data, hit_w.ctypes.data, None, None), "kmpgpu_scan_regexes")
            assert np.array_equal(hit_w, MM.words(rows)) and np.array_equal(any_w, MM.words(rows.any(axis=0)))
    finally:
        reset(gm)


@pytest.mark.parametrize("whole", [False, True])
def test_gates_same_verdicts_and_all_flagged(gm, world, whole):
    body = GROUPED[:4]
    gated = [g(e, gate=q) for q in range(4) for e in body]            # pattern 3 is in no payload
    same = [x for e in LINEAR for x in (e, g(e))] + [x for e in body for x in (g(e), g(e, nocase=True))]
    reset(gm)
    try:
        _setup(gm, world.payloads, gated + [g(e) for e in body], whole)
        rows = world.rows(gated + [g(e) for e in body], whole)
        # the gate nobody holds empties its rows; the others take payloads away from some rows and leave some in most
        assert not rows[12:16].any() and (rows[:12].sum(axis=1) > 0).sum() >= 6
        assert all(r.sum() <= f.sum() for q in range(3) for r, f in zip(rows[4 * q:4 * q + 4], rows[16:])) and rows[:12].sum() < 3 * rows[16:].sum()
        res = _check(gm, rows)
        # every expression flagged: the grouped kernel alone stands in the reduce's place
        assert res["timing"].launches == gm.scan_packets()["timing"].launches
        gm.set_regexes(same)
        rows = world.rows(same, whole)
        got = _check(gm, rows)["hits"]
        for i in range(len(LINEAR)):
            assert np.array_equal(got[2 * i], got[2 * i + 1])
        # a mixed set is one launch more
        assert gm.scan_regexes()["timing"].launches == gm.scan_packets()["timing"].launches + 1
    finally:
        reset(gm)


def test_as_rule_terms_and_profile(gm, world):
    """A profile records durations, not names, so the order of the launches is pinned by what they compute: the linear kernel stores
    zeros into a flagged expression's row, so a grouped launch in front of it would leave that row empty, and the rules kernel reads the
    rows, so a grouped launch behind it would leave the rules without them.  Both rows are non-trivial here."""
    exprs = [LINEAR[0], g(GROUPED[0]), g(GROUPED[1], gate=0)]
    xrows = world.rows(exprs)
    mat = np.concatenate([world.hits[False], xrows])
    x0 = len(PATS)
    rules = [([x0 + 1], []), ([0], [x0 + 1]), ([], [x0 + 2, x0 + 0]), ([x0 + 0, x0 + 1], [x0 + 2])]
    want = MM.rule_rows(mat, rules)
    assert want.any(axis=1).all() and 0 < want.sum() < want.size
    reset(gm)
    try:
        _setup(gm, world.payloads, exprs)
        gm.set_rules(rules)
        res = gm.scan_rules(hits=True)
        assert np.array_equal(res["hits"], want) and res["rule_pkt_counts"].tolist() == want.sum(axis=1).tolist()
        al = gm.scan_alerts("rules")
        assert [(int(a["packet"]), int(a["index"])) for a in al["alerts"]] == sorted((int(k), int(r)) for r, k in np.argwhere(want))

        def launches(ex):
            gm.set_regexes(ex)
            gm.set_rules(rules)
            gm.profile_begin(64)
            gm.scan_rules()
            return len(gm.profile_end(64))

        unflagged = launches([LINEAR[0], LINEAR[1], LINEAR[2]])
        assert launches(exprs) == unflagged + 1                                     # mixed: the grouped launch behind the linear one
        assert launches([g(e) for e in GROUPED[:3]]) == unflagged                  # all flagged: no linear launch
    finally:
        reset(gm)


def test_refusals_keep_the_earlier_set(gm, world):
    n = 100
    keep = [g(GROUPED[0]), LINEAR[0]]
    rows = world.rows(keep, False, n)
    reset(gm)
    try:
        _setup(gm, world.payloads[:n], keep)
        for bad, what in ((b"(a|)", "expression 1: position 3: an empty alternative"), (b"()", "expression 1: position 0: an empty group"),
                          (b"a||b", "expression 1: position 2: an empty alternative"), (b"|a", "expression 1: position 0: an empty alternative"),
                          (b"^a|b", "expression 1: position 2: a top-level '\\|' beside \\^ or \\$ \\(write \\^\\(a\\|b\\)\\$"),
                          (b"(?=a)", "expression 1: position 0: '\\(\\?' opens no group but \\(\\?:"), (b"(a", "expression 1: position 0: unterminated group"),
                          (b"a)", "expression 1: position 1: '\\)' without its opening"), (b"(a)+?", "expression 1: position 4: a quantifier on a quantifier"),
                          (b"(a{8}){8}", "expression 1: position 0: more than 63 positions"),
                          (b"(ab|cd){2,5}e", "expression 1: position 0: needs 9 edge rules, more than 8")):
            with raises(EINVAL, what):
                gm.set_regexes([b"ok", g(bad)])
        with raises(EINVAL, "expression 0: position 1: '\\(' is reserved"):
            gm.set_regexes([b"a(b)"])
        _check(gm, rows)
    finally:
        reset(gm)
