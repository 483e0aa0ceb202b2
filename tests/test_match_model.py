"""tests/match_model.py, the host model behind the GPU tests' exact comparisons, held to the CPU oracle and to definitions written
out here.  No GPU."""
import json
import os
import random

import numpy as np
import pytest

import match_model as MM
import multithreading_string_matching_amd as K
from conftest import DATA, GOLDEN

ALPHABET = b"abAB"
LENGTHS = [1, 2, 3, 4, 5, 16, 17, 40]
MAX_LEN = 200
U32_MAX = 0xFFFFFFFF


def _flip(rng, p):
    return bytes(c ^ 0x20 if rng.random() < 0.3 else c for c in p)       # (the alphabet is letters only)


@pytest.fixture(scope="module")
def case():
    """(payloads, patterns): 40 payloads without a 0x00, the patterns cut from them, then 400 payloads of 0..200 bytes with the patterns
    planted in either case and a 0x00 at byte 0, at the last byte, directly before, inside or behind a planted occurrence, or nowhere"""
    rng = random.Random("match-model")
    payloads = [bytes(rng.choice(ALPHABET) for _ in range(rng.randrange(60, MAX_LEN + 1))) for _ in range(40)]
    pats = [b"aa", b"abab", b"a", b"B"]                                   # self-overlapping ones, and both cases of a 1-byte one
    for m in LENGTHS:
        for _ in range(2):
            t = rng.choice(payloads)
            s = rng.randrange(len(t) - m + 1)
            pats.append(t[s:s + m])
    payloads += [b"", b"\0", b"a", b"\0a", b"a\0", b"aaaa", b"aaaa\0aa", b"ababab", b"abAbaBab\0abab", pats[-1], pats[-1][:-1]]
    for k in range(400):
        L = 0 if k % 40 == 0 else rng.randrange(1, MAX_LEN + 1)
        b = bytearray(rng.choice(ALPHABET) for _ in range(L))
        planted = []
        for _ in range(rng.randrange(1, 4)):
            p = _flip(rng, rng.choice(pats + [b"aaaaa", b"abababab"]))
            if len(p) <= L:
                s = rng.randrange(L - len(p) + 1)
                b[s:s + len(p)] = p
                planted.append((s, len(p)))
        s, m = rng.choice(planted) if planted else (0, 1)
        kind = ("none", "first", "last", "before", "inside", "behind")[k % 6]
        if L and kind == "first":
            b[0] = 0
        elif L and kind == "last":
            b[L - 1] = 0
        elif kind == "before" and s > 0:
            b[s - 1] = 0
        elif L and kind == "inside":
            b[s + rng.randrange(m)] = 0
        elif kind == "behind" and s + m < L:
            b[s + m] = 0
        payloads.append(bytes(b))
    assert sorted({len(p) for p in pats}) == LENGTHS and b"" in payloads
    return payloads, pats


def test_fold_and_text_end():
    every = bytes(range(256))
    want = bytes(c + 0x20 if 0x41 <= c <= 0x5A else c for c in every)
    assert MM.fold(every) == MM.fold(bytearray(every)) == want
    arr = np.frombuffer(every, dtype=np.uint8)
    assert MM.fold(arr).tobytes() == want and arr.tobytes() == every      # a copy: the input stays
    for t, e in ((b"", 0), (b"\0", 0), (b"ab", 2), (b"ab\0", 2), (b"a\0b\0", 1)):
        assert MM.text_end(t) == e and MM.text_end(t, whole=True) == len(t)


def test_counts_equal_the_oracle(oracle, case):
    payloads, pats = case
    flags = [i % 2 == 0 for i in range(len(pats))]
    plain = [int(x) for x in oracle.count_payloads(payloads, pats)]
    folded = [int(x) for x in oracle.count_payloads([t.lower() for t in payloads], [p.lower() for p in pats])]
    remapped = [int(x) for x in oracle.count_payloads([t.replace(b"\0", b"\xff") for t in payloads], pats)]
    both = [int(x) for x in oracle.count_payloads([t.replace(b"\0", b"\xff").lower() for t in payloads], [p.lower() for p in pats])]
    mixed = [f if nc else c for f, c, nc in zip(folded, plain, flags)]
    assert plain != folded and plain != remapped and all(c > 0 for c in plain[:4])        # the input tells the rules apart
    assert MM.counts(MM.starts(payloads, pats)) == plain
    assert MM.counts(MM.starts(payloads, pats, nocase=[True] * len(pats))) == folded
    assert MM.counts(MM.starts(payloads, pats, nocase=flags)) == mixed
    assert MM.counts(MM.starts(payloads, pats, whole=True)) == remapped
    assert MM.counts(MM.starts(payloads, pats, nocase=[True] * len(pats), whole=True)) == both
    # the oracle's side of the GPU tests, by both of its entry points
    assert MM.oracle_counts(oracle, payloads, pats) == plain
    assert MM.oracle_counts(oracle, payloads, pats, nocase=True) == folded
    assert MM.oracle_counts(oracle, payloads, pats, nocase=flags) == mixed
    assert MM.oracle_counts(oracle, payloads, pats, whole=True) == remapped
    assert MM.oracle_counts(oracle, payloads, pats, nocase=True, whole=True) == both
    arena = K.HostArena.from_payloads(payloads)
    for nocase, whole, want in ((None, False, plain), (flags, False, mixed), (None, True, remapped), (True, True, both)):
        assert MM.oracle_counts_arena(oracle, arena.bytes, arena.off, arena.len, pats, nocase, whole) == want
    with pytest.raises(AssertionError):
        MM.oracle_counts(oracle, payloads, pats + [b"a\xff"], whole=True)


def test_derived_views(case):
    payloads, pats = case
    st = MM.starts(payloads, pats)
    assert all(ss == sorted(set(ss)) for row in st for ss in row)
    recs = MM.records(st)
    assert len(recs) == sum(MM.counts(st))
    assert all(payloads[k][s:s + len(pats[i])] == pats[i] and s + len(pats[i]) <= MM.text_end(payloads[k]) for k, s, i in recs)
    hits = MM.hits(st)
    assert hits.shape == (len(pats), len(payloads)) and hits.dtype == bool
    assert {(k, i) for k, _, i in recs} == {(int(k), int(i)) for i, k in np.argwhere(hits)}
    assert MM.counts(st) == [sum(1 for _, _, i in recs if i == j) for j in range(len(pats))]
    assert MM.per_payload(st).sum() == len(recs) and MM.per_payload(st)[1].tolist() == [len(row[1]) for row in st]
    # overlapping starts, by hand
    assert MM.starts([b"aaaa", b"ababab\0abab", b""], [b"aa", b"abab"]) == [[[0, 1, 2], []], [[], [0, 2]], [[], []]]
    assert MM.starts([b"ababab\0abab"], [b"abab"], whole=True) == [[[0, 2, 7]]]
    assert MM.starts([b"aAaa"], [b"Aa", b"Aa"], nocase=[True, False]) == [[[0, 1, 2], [1]]]
    assert MM.hits([], 3).shape == (3, 0) and MM.counts([], 3) == [0, 0, 0] and MM.hits(MM.starts(payloads, [])).shape == (0, len(payloads))
    rec = np.array([(7, 3, 1), (2, 9, 0)], dtype=[("packet", np.uint32), ("offset", np.uint32), ("pattern", np.uint32)])
    assert MM.triples(rec) == [(2, 9, 0), (7, 3, 1)]


@pytest.mark.parametrize("nocase,whole", [(False, False), (True, False), (False, True)])
def test_windows_filter_the_starts(case, nocase, whole):
    payloads, pats = case
    flags = [nocase] * len(pats)
    free = MM.starts(payloads, pats, nocase=flags, whole=whole)
    assert MM.starts(payloads, pats, [], flags, whole) == free and MM.starts(payloads, pats, [(0, None)] * len(pats), flags, whole) == free
    known = [next(ss[-1] for row in free for ss in [row[i]] if ss) for i in range(len(pats))]          # a start of every pattern
    for turn in range(5):
        kinds = [[(0, 0), (0, None), (known[i], known[i]), (MAX_LEN + 1, MAX_LEN + 100), (0, U32_MAX - 1)][(i + turn) % 5] for i in range(len(pats))]
        got = MM.starts(payloads, pats, kinds, flags, whole)
        want = [[[s for s in ss if a <= s <= (U32_MAX if b is None else b)] for ss, (a, b) in zip(row, kinds)] for row in free]
        assert got == want
        for i, (a, b) in enumerate(kinds):
            col = [row[i] for row in got]
            if (a, b) == (MAX_LEN + 1, MAX_LEN + 100):
                assert not any(col)                                       # behind every payload
            elif a == b:
                assert (any(col) or a != known[i]) and all(ss in ([], [a]) for ss in col)
            else:
                assert col == [row[i] for row in free]
    with pytest.raises(AssertionError):
        MM.starts(payloads, pats, [(0, 0)])


def test_relation_rows_against_the_definition():
    A, B, P, Q = b"EFX", b"GHY", b"PQRS", b"RSTU"
    pats = [A, B, P, Q]

    def text(L, items):
        b = bytearray(b"abcd"[i % 4] for i in range(L))
        for s, p in items:
            b[s:s + len(p)] = p
        return bytes(b)

    payloads = [text(60, [(10, A), (20, B)]),                 # d = 7
                text(60, [(10, A), (13, B)]),                 # d = 0: B directly behind A
                text(60, [(20, A), (10, B)]),                 # d = -13: B in front of A
                text(60, [(5, b"PQRSTU")]),                   # Q starts inside P: d = -2
                text(80, [(10, A), (30, A), (34, B), (70, A)]),       # d = 21, 1, -39
                text(80, [(10, A), (40, A)]),                 # a == b: d = -3 with itself, 27 and -33 with the other
                text(60, [(10, A)]), text(60, [(20, B)]), b"",
                text(60, [(10, A), (20, B)])[:18] + b"\0" + text(60, [(10, A), (20, B)])[19:]]       # the 0x00 cuts B off
    relations = [(0, 1, 7, 7), (0, 1, 8, 9), (0, 1, 5, 6), (0, 1, 6, 8), (0, 1, 0, 0), (0, 1, 1, 1), (0, 1, -1, -1),
                 (0, 1, -13, -13), (0, 1, -12, -1), (0, 1, -20, -14), (0, 1, None, -1), (0, 1, 0, None), (0, 1, None, None),
                 (1, 0, -13, -13), (1, 0, 7, 7), (2, 3, -2, -2), (2, 3, -1, 0), (2, 3, -3, -3), (3, 2, -6, -6),
                 (0, 1, 21, 21), (0, 1, 2, 20), (0, 1, -39, -39), (0, 1, -38, 0), (0, 0, -3, -3), (0, 0, 27, 27), (0, 0, -33, -33),
                 (0, 0, 0, 26), (0, 0, -2, -1), (0, 0, 28, None), (0, 1, 7, 7)]
    st = MM.starts(payloads, pats)
    got = MM.relation_rows(st, pats, relations)
    want = np.zeros_like(got)
    for k, raw in enumerate(payloads):                                    # the definition: every pair of offsets of the text
        t = raw[:MM.text_end(raw)]
        for q, (a, b, lo, hi) in enumerate(relations):
            for sa in range(len(t)):
                for sb in range(len(t)):
                    d = sb - (sa + len(pats[a]))
                    if t.startswith(pats[a], sa) and t.startswith(pats[b], sb) and (lo is None or lo <= d) and (hi is None or d <= hi):
                        want[q, k] = True
    assert got.shape == (len(relations), len(payloads)) and (got == want).all(), np.argwhere(got != want)[:8].tolist()
    # and a few cells by hand: the bound met, one byte outside on either side, in front, overlapping, with itself
    col = {q: got[q].nonzero()[0].tolist() for q in range(len(relations))}
    assert col[0] == [0] and col[1] == [] and col[2] == [] and col[3] == [0] and col[4] == [1] and col[5] == [4] and col[6] == []
    assert col[7] == [2] and col[8] == [] and col[9] == [] and col[10] == [2, 4] and col[11] == [0, 1, 4] and col[12] == [0, 1, 2, 4]
    assert col[13] == [0] and col[14] == [2] and col[15] == [3] and col[16] == [] and col[17] == [] and col[18] == [3]
    assert col[23] == [0, 1, 2, 4, 5, 6, 9] and col[24] == [5] and col[25] == [5] and col[26] == [4] and col[27] == [] and col[28] == [4]
    assert (got[29] == got[0]).all()                                      # the same relation twice
    assert MM.pair_exists([4], [9], 3, 2, 2) and not MM.pair_exists([4], [9], 3, 3, None) and not MM.pair_exists([], [9], 3, None, None)
    # windows and the text's end decide what a start is
    assert not MM.relation_rows(MM.starts(payloads, pats, [(11, None), (0, None), (0, None), (0, None)]), pats, relations)[0].any()
    assert MM.relation_rows(MM.starts(payloads, pats, whole=True), pats, relations)[0].nonzero()[0].tolist() == [0, 9]


def test_rule_rows_and_flat_rules():
    mat = np.array([[1, 1, 0, 0], [1, 0, 1, 0], [0, 0, 0, 1]], dtype=bool)
    rules = [([0], []), ([0, 1], []), ([0], [1]), ([], [0, 1]), ([2], [2]), ([], [2, 2]), ([0, 0], [])]
    rows = MM.rule_rows(mat, rules)
    assert rows.astype(int).tolist() == [[1, 1, 0, 0], [1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1], [0, 0, 0, 0], [1, 1, 1, 0], [1, 1, 0, 0]]
    assert MM.rule_rows(mat, []).shape == (0, 4)
    off, terms = MM.flat_rules(rules)
    assert off.tolist() == [0, 1, 3, 5, 7, 9, 11, 13] and off.dtype == terms.dtype == np.uint32
    N = MM.RULE_NOT
    assert terms.tolist() == [0, 0, 1, 0, 1 | N, 0 | N, 1 | N, 2, 2 | N, 2 | N, 2 | N, 0, 0]
    assert MM.flat_rules([])[0].tolist() == [0]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_words_round_trip(n):
    bits = np.random.default_rng(n).random((3, n)) < 0.5
    bits[0] = True
    w = MM.words(bits)
    assert w.dtype == np.uint64 and w.shape == (3, (n + 63) // 64)
    back = np.unpackbits(w.view(np.uint8), axis=-1, bitorder="little").astype(bool)
    assert (back[:, :n] == bits).all() and not back[:, n:].any()
    assert int(MM.words(bits[0])[0]) == (1 << min(n, 64)) - 1                     # LSB first


def test_committed_capture(tokens, fixture_counts):
    arena = K.HostArena.from_pcap(os.path.join(DATA, "udp_1000.pcap"), "udp")
    payloads = [arena.payload(k) for k in range(arena.n_pkts)]
    with open(os.path.join(GOLDEN, "whole_payload_counts.json")) as f:
        whole = json.load(f)["fixtures"]["udp_1000.pcap:udp"]["counts"]
    today = fixture_counts["fixtures"]["udp_1000.pcap:udp"]["counts"]
    assert MM.counts(MM.starts(payloads, tokens)) == today
    assert MM.counts(MM.starts(payloads, tokens, whole=True)) == whole and whole != today
