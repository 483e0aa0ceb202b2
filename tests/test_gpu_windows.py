"""Per-pattern offset windows (kmpgpu_set_windows, GpuMatcher.set_windows) on a real MI355X.

The expectation is the host model of tests/match_model.py: the starts inside the patterns' windows are the records, their (pattern,
payload) pairs the hit matrix, from which pkt_counts, any and the rule rows follow.  counts -- which the windows must not touch --
come from the CPU oracle.  Every comparison is exact.

Run on a real MI355X:  python -m pytest tests/test_gpu_windows.py -m gpu
"""
import os
import random

import numpy as np
import pytest

from conftest import DATA, GOLDEN

pytestmark = pytest.mark.gpu

from gpu_support import KERNELS, check_offsets, check_packets, check_rules, gm, reset, run_cli, strip_elapsed  # noqa: E402,F401  (torch first)

import match_model as MM  # noqa: E402
import multithreading_string_matching_amd as K  # noqa: E402
from match_model import U32_MAX  # noqa: E402
from multithreading_string_matching_amd import _lib  # noqa: E402
from multithreading_string_matching_amd.matcher import OPT_ACCUMULATE, OPT_FUSED, OPT_KERNEL, OPT_REPACK, OPT_WHOLE_PAYLOAD, GpuMatcher  # noqa: E402

ALPHABET = b"abcdAB"
BEHIND = (5000, 6000)                                # behind the end of every payload of these tests (at most 2200 bytes)


def check_all(gm, oracle, payloads, pats, windows, rules=None, nocase=None, whole=False, kernels=KERNELS):
    """the three calls that follow the windows, and the counts that do not, on every kernel setting"""
    st = MM.starts(payloads, pats, windows, nocase, whole)
    recs, hits = MM.records(st), MM.hits(st, len(pats))
    counts = MM.oracle_counts(oracle, payloads, pats, nocase, whole)
    for name, kernel, fused in kernels:
        gm.set_option(OPT_KERNEL, kernel); gm.set_option(OPT_FUSED, fused)
        check_offsets(gm, recs, counts)
        check_packets(gm, hits, counts)
        if rules:
            check_rules(gm, hits, rules, counts)
        assert gm.scan()[0].tolist() == counts, name
    return recs, hits, counts


# ------------------------------------------------------------------------------------------------
# arenas, as tests/test_gpu_packets.py builds them
# ------------------------------------------------------------------------------------------------
def make_payloads(rng, kind, plant, n=300):
    if kind == "uniform":
        lens = [1500] * n
    else:
        lens = [0 if rng.random() < 0.1 else rng.randrange(0, 2200) for _ in range(n)]
    payloads = []
    for L in lens:
        b = bytearray(rng.choice(ALPHABET) for _ in range(L))
        for _ in range(L // 100):                    # plant patterns so that most of them hit somewhere, many times
            p = rng.choice(plant)
            if len(p) <= L:
                s = rng.randrange(L - len(p) + 1)
                b[s:s + len(p)] = p
        if L:                                        # and at the head, where the anchored windows look
            p = rng.choice(plant)
            s = rng.choice([0, 0, 1, 15, 16, 17])
            if s + len(p) <= L:
                b[s:s + len(p)] = p
        payloads.append(bytes(b))
    return payloads


def sub(rng, payloads, m):
    """a piece of some payload's text (so that it matches)"""
    for _ in range(200):
        t = rng.choice(payloads)
        t = t[:MM.text_end(t)]
        if len(t) >= m:
            s = rng.randrange(len(t) - m + 1)
            return t[s:s + m]
    return bytes(rng.choice(ALPHABET) for _ in range(m))


def load_in_place_dirty(gm, rng, payloads, plant):
    """OPT_REPACK = 0: slots with gaps, not in payload order, and padding and gaps that continue with text that would complete
    a match.  The offsets / marking pass packs such an arena on the call."""
    ln = np.array([len(t) for t in payloads], dtype=np.uint32)
    slot = np.maximum(16, (ln.astype(np.uint64) + 15) // 16 * 16) + 32
    order = list(range(len(payloads)))
    rng.shuffle(order)
    off = np.zeros(len(payloads), dtype=np.uint64)
    pos = 0
    for k in order:
        off[k] = pos
        pos += int(slot[k])
    fill = (b"".join(plant) * (pos // sum(len(p) for p in plant) + 2))[:pos]
    arena = np.frombuffer(fill + b"\0" * 64, dtype=np.uint8).copy()
    for k, t in enumerate(payloads):
        arena[int(off[k]):int(off[k]) + len(t)] = np.frombuffer(t, dtype=np.uint8)
    gm.set_option(OPT_REPACK, 0)
    gm.load_arena(arena, off, ln)


WINDOW_KINDS = [(0, 0), (0, None), (0, U32_MAX), (0, 63), (16, 16), (17, 1023), (1024, None), (1, 15), (1025, 1500), BEHIND, (0, U32_MAX - 1)]


def random_windows(rng, n):
    out = []
    for _ in range(n):
        if rng.random() < 0.3:
            a = rng.randrange(0, 1600)
            out.append((a, a + rng.randrange(0, 600)))
        else:
            out.append(rng.choice(WINDOW_KINDS))
    return out


def random_rules(rng, n_pat, n=6):
    rules = []
    for _ in range(n):
        pos = [rng.randrange(n_pat) for _ in range(rng.randrange(0, 3))]
        neg = [rng.randrange(n_pat) for _ in range(rng.randrange(0, 2) if pos else 1)]
        rules.append((pos, neg))
    return rules


# ------------------------------------------------------------------------------------------------
# 1. every kernel family: offsets, packets, rules
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["uniform", "mixed", "in_place_dirty"])
def test_every_kernel_family(gm, oracle, kind):
    rng = random.Random(f"windows-{kind}")
    plant = [bytes(rng.choice(ALPHABET) for _ in range(m)) for m in (2, 3, 5, 9, 17, 40)]
    payloads = make_payloads(rng, "uniform" if kind == "uniform" else "mixed", plant)
    pats = plant + [sub(rng, payloads, m) for m in (1, 4, 8, 16)] + [plant[1], plant[3]]
    windows = random_windows(rng, len(pats))
    windows[0], windows[3] = (0, 0), (1023, 1025)
    rules = random_rules(rng, len(pats))
    try:
        reset(gm)
        gm.set_patterns(pats)
        if kind == "in_place_dirty":
            load_in_place_dirty(gm, rng, payloads, plant)
        else:
            gm.load_arena(K.HostArena.from_payloads(payloads))
        gm.set_windows(windows)
        gm.set_rules(rules)
        assert gm.windows == [(a, b) for a, b in windows]
        recs, hits, counts = check_all(gm, oracle, payloads, pats, windows, rules)
        # the windows did something, and not everything
        assert 0 < len(recs) < sum(counts) and hits.any()
    finally:
        reset(gm)


# ------------------------------------------------------------------------------------------------
# 2. pattern lengths x window edges: planted at first - 1, first, last, last + 1
# ------------------------------------------------------------------------------------------------
LENGTHS = [1, 2, 3, 4, 5, 8, 9, 16, 17, 40, 99]


def edge_windows(L, m):
    last_start = L - m
    return [(0, 0), (15, 15), (16, 16), (17, 17), (15, 17), (1, 16), (1023, 1023), (1024, 1024), (1025, 1025), (1023, 1025), (16, 1024),
            (last_start, last_start), (last_start, None), (last_start - 1, last_start + 7), BEHIND, (0, U32_MAX), (0, U32_MAX - 1)]


def planted_payloads(rng, lens, pats_windows):
    """one payload per (pattern, window, edge): the pattern at first - 1, first, last or last + 1 where it fits the payload, in text
    that holds none of the patterns' letters; then a few payloads with a pattern at every one of their edges"""
    jobs = [(p, s) for p, (a, b) in pats_windows for s in (a - 1, a, (a if b is None or b >= U32_MAX - 1 else b), (a if b is None or b >= U32_MAX - 1 else b) + 1)]
    payloads = []
    for n, L in enumerate(lens):
        b = bytearray(rng.choice(b"abcd") for _ in range(L))
        if n < len(jobs):
            p, s = jobs[n]
            if 0 <= s and s + len(p) <= L:
                b[s:s + len(p)] = p
        else:
            p = pats_windows[n % len(pats_windows)][0]
            for s in (0, 16, 1024 - len(p), 1023, L - len(p)):          # also across the chunk edge, and the payload's last start
                if 0 <= s and s + len(p) <= L:
                    b[s:s + len(p)] = p
        payloads.append(bytes(b))
    return payloads


@pytest.mark.parametrize("uniform", [True, False], ids=["uniform", "mixed"])
@pytest.mark.parametrize("m", LENGTHS)
def test_lengths_and_edges(gm, oracle, m, uniform):
    rng = random.Random(f"edges-{m}-{uniform}")
    L = 1500
    P = bytes(rng.choice(b"EFGH") for _ in range(m - 1)) + b"X"
    Q = bytes(rng.choice(b"EFGH") for _ in range(m - 1)) + b"Y"
    wins = edge_windows(L, m)
    # every window on both patterns (two distinct patterns: the fused pass takes them, 1-byte ones as riders), each window an index of its own
    pats = [P] * len(wins) + [Q] * len(wins) + [b"a" * m]
    windows = wins + wins + [(16, 1030)]
    n = 4 * 2 * len(wins) + 24
    lens = [L] * n if uniform else [rng.randrange(1030 + m, 2200) for _ in range(n)]
    payloads = planted_payloads(rng, lens, list(zip(pats[:-1], windows[:-1])))
    payloads += [b"a" * (L if uniform else 1100 + 7 * j) for j in range(4)]          # dense: the last pattern at every offset
    if not uniform:
        payloads += [b"", P, b"a" * m, Q + P]                                         # short ones: a match at offset 0 and nothing else
    try:
        reset(gm)
        gm.set_patterns(pats)
        gm.load_arena(K.HostArena.from_payloads(payloads))
        gm.set_windows(windows)
        recs, hits, counts = check_all(gm, oracle, payloads, pats, windows)
        nw = len(wins)
        assert not hits[wins.index(BEHIND)].any() and not hits[nw + wins.index(BEHIND)].any()      # wholly behind every payload: never
        assert hits[0].any() and hits[wins.index((1024, 1024))].any()
        # [0, UINT32_MAX] on an index = no window on it
        free = MM.hits(MM.starts(payloads, pats))
        assert (hits[wins.index((0, U32_MAX))] == free[0]).all() and (hits[wins.index((0, U32_MAX - 1))] == free[0]).all()
        assert (hits[0] != free[0]).any()
    finally:
        reset(gm)


# ------------------------------------------------------------------------------------------------
# 3. the fused pass: classed groups, 1-byte riders, duplicates with a window each
# ------------------------------------------------------------------------------------------------
def test_fused_classed_group(gm, oracle):
    rng = random.Random("classed")
    plant = [bytes(rng.choice(ALPHABET) for _ in range(m)) for m in (4, 5, 6, 8)]
    payloads = make_payloads(rng, "mixed", plant)
    seen, pats = set(), []
    while len(pats) < 300:
        p = sub(rng, payloads, rng.choice([4, 5, 6, 8]))
        if p not in seen and b"\0" not in p:
            seen.add(p); pats.append(p)
    windows = random_windows(rng, len(pats))
    rules = random_rules(rng, len(pats), 8)
    try:
        reset(gm)
        gm.set_patterns(pats)
        gm.load_arena(K.HostArena.from_payloads(payloads))
        gm.set_windows(windows)
        gm.set_rules(rules)
        recs, _, counts = check_all(gm, oracle, payloads, pats, windows, rules, kernels=[KERNELS[0], KERNELS[2]])
        assert 0 < len(recs) < sum(counts)
    finally:
        reset(gm)


def test_fused_one_byte_patterns(gm, oracle):
    """six 1-byte patterns: four ride along with the fused group, two get reads of their own"""
    rng = random.Random("riders")
    plant = [bytes(rng.choice(ALPHABET) for _ in range(m)) for m in (2, 5, 9)]
    payloads = make_payloads(rng, "mixed", plant, n=200)
    pats = [b"a", b"B", b"c", b"d", b"A", b"b"] + plant + [b"a", b"b"]
    windows = [(0, 0), (15, 17), (1023, 1025), (0, None), (16, 16), (1, 40), (0, 63), (17, 1030), (0, 0), BEHIND, (1024, None)]
    rules = [([0, 4], [1]), ([9], []), ([10], [5]), ([], [0])]
    try:
        reset(gm)
        gm.set_patterns(pats)
        gm.load_arena(K.HostArena.from_payloads(payloads))
        gm.set_windows(windows)
        gm.set_rules(rules)
        check_all(gm, oracle, payloads, pats, windows, rules)
    finally:
        reset(gm)


def test_duplicates_with_a_window_each(gm, oracle):
    """the same bytes three times, three windows: three rows, three sets of records, and one rule over all three"""
    rng = random.Random("dups")
    tok = b"GET /"
    payloads = []
    for k in range(260):
        L = rng.randrange(40, 1800)
        b = bytearray(rng.choice(b"abcd ") for _ in range(L))
        for s in ([0] if k % 2 else []) + ([rng.randrange(8, 33)] if k % 3 == 0 else []) + ([rng.randrange(100, L)] if k % 5 == 0 and L > 200 else []):
            if s + len(tok) <= L:
                b[s:s + len(tok)] = tok
        payloads.append(bytes(b))
    pats = [tok, b"ab", tok, b"cd a", tok]
    windows = [(0, 0), (0, None), (8, 32), (0, 700), (100, None)]
    rules = [([0, 2], [4]), ([0], [2]), ([4], [0, 2]), ([0, 2, 4], [])]          # the first: two of the duplicates, and not the third
    try:
        reset(gm)
        gm.set_patterns(pats)
        gm.load_arena(K.HostArena.from_payloads(payloads))
        gm.set_windows(windows)
        gm.set_rules(rules)
        recs, hits, counts = check_all(gm, oracle, payloads, pats, windows, rules)
        assert counts[0] == counts[2] == counts[4]
        rows = [hits[i].tolist() for i in (0, 2, 4)]
        assert rows[0] != rows[1] and rows[1] != rows[2] and rows[0] != rows[2]
        assert MM.rule_rows(hits, rules).sum(axis=1).min() > 0
    finally:
        reset(gm)


# ------------------------------------------------------------------------------------------------
# 4. composition: nocase, whole payloads, windows as pass state
# ------------------------------------------------------------------------------------------------
def test_with_nocase_mixed_flags(gm, oracle):
    rng = random.Random("nocase")
    plant = [b"ABab", b"aBc", b"dAbCa", bytes(rng.choice(ALPHABET) for _ in range(17))]
    payloads = make_payloads(rng, "mixed", plant)
    pats = plant + [sub(rng, payloads, m) for m in (1, 2, 6, 16)] + [b"abab", b"ABAB"]
    nocase = [True, False, True, True, True, False, True, False, True, False]
    windows = [(0, 17), (0, 0), (16, None), (1, 1024), (0, 0), (1023, 1025), (0, 63), BEHIND, (0, 16), (0, None)]
    rules = [([0, 8], []), ([0], [9]), ([2, 3], [1])]
    try:
        reset(gm)
        gm.set_patterns(pats, nocase=nocase)
        gm.load_arena(K.HostArena.from_payloads(payloads))
        gm.set_windows(windows)
        gm.set_rules(rules)
        recs, hits, _ = check_all(gm, oracle, payloads, pats, windows, rules, nocase=nocase)
        assert hits[0].sum() > MM.hits(MM.starts(payloads, pats, windows))[0].sum()           # folding found more inside the window
    finally:
        reset(gm)


def test_with_whole_payload(gm, oracle):
    """a 0x00 inside the window's range: the match behind it is in window only with OPT_WHOLE_PAYLOAD"""
    rng = random.Random("whole")
    pats = [b"XY", b"XYZW_", b"Z", b"XYZW_longer_than_16b", b"XY"]
    windows = [(20, 60), (0, 1100), (1000, None), (16, 1030), (0, 10)]
    rules = [([0], [4]), ([1, 2], []), ([], [3])]
    payloads = []
    for k in range(240):
        L = 1500 if k < 100 else rng.randrange(80, 2100)
        b = bytearray(rng.choice(b"abcd") for _ in range(L))
        for p, (a, last) in zip(pats, windows):
            s = a + rng.randrange(50)
            if s + len(p) <= L and rng.random() < 0.6:
                b[s:s + len(p)] = p
        if k % 3:
            b[rng.choice([5, 15, 16, 30, 999, 1023, 1024])  % L] = 0
        payloads.append(bytes(b))
    try:
        reset(gm)
        gm.set_patterns(pats)
        gm.load_arena(K.HostArena.from_payloads(payloads))
        gm.set_windows(windows)
        gm.set_rules(rules)
        seen = {}
        for whole in (0, 1, 0):
            gm.set_option(OPT_WHOLE_PAYLOAD, whole)
            seen[whole] = check_all(gm, oracle, payloads, pats, windows, rules, whole=bool(whole))[0]
        assert seen[0] < seen[1]                                                      # a proper subset
    finally:
        reset(gm)


def test_windows_are_pass_state(gm, oracle):
    """changed and cleared between two passes of one context, nothing reloaded; cleared = a fresh context, bit for bit"""
    rng = random.Random("state")
    plant = [bytes(rng.choice(ALPHABET) for _ in range(m)) for m in (3, 6, 17)]
    payloads = make_payloads(rng, "mixed", plant, n=200)
    pats = plant + [b"a", b"ab"]
    rules = [([0, 1], []), ([4], [2])]
    g = _lib.gpu_lib()

    def raw(m):
        """every output of the three calls, as the C-ABI writes them"""
        out = []
        for _, kernel, fused in KERNELS:
            m.set_option(OPT_KERNEL, kernel); m.set_option(OPT_FUSED, fused)
            recs, found, cnt = m.scan_offsets(4_000_000)
            pk = m.scan_packets(hits=True)
            ru = m.scan_rules(hits=True)
            out.append((MM.triples(recs), found, cnt.tolist(), pk["hits"].tobytes(), pk["pkt_counts"].tolist(), pk["any"].tobytes(), pk["counts"].tolist(),
                        ru["hits"].tobytes(), ru["rule_pkt_counts"].tolist(), ru["any"].tobytes(), ru["counts"].tolist(), m.scan()[0].tolist()))
        return out

    try:
        reset(gm)
        with GpuMatcher(0) as fresh:
            fresh.set_patterns(pats)
            fresh.load_arena(K.HostArena.from_payloads(payloads))
            fresh.set_rules(rules)
            base = raw(fresh)
        gm.set_patterns(pats)
        gm.load_arena(K.HostArena.from_payloads(payloads))
        gm.set_rules(rules)
        assert raw(gm) == base
        w1 = [(0, 0), (16, 1024), (0, None), (5, 5), BEHIND]
        w2 = [(1, None), (0, 15), (1025, 1300), (0, None), (0, 0)]
        for w in (w1, w2, w1):
            gm.set_windows(w)
            check_all(gm, oracle, payloads, pats, w, rules)
        # all-default windows, then cleared three ways: as if never set
        for clear in ([(0, None)] * len(pats), [(0, U32_MAX)] * len(pats), None, [], "abi"):
            gm.set_windows(w2)
            if clear == "abi":
                assert g.kmpgpu_set_windows(gm._ctx, None, None, 0) == 0
            else:
                gm.set_windows(clear)
                assert gm.windows == list(clear or [])
            assert raw(gm) == base, clear
    finally:
        reset(gm)


# ------------------------------------------------------------------------------------------------
# 5. what must not move: the context's own counters
# ------------------------------------------------------------------------------------------------
def test_counters_are_untouched(gm, oracle):
    rng = random.Random("acc")
    plant = [b"abca", b"dd", b"Ab"]
    payloads = make_payloads(rng, "mixed", plant, n=200)
    pats = plant + [b"a"]
    windows = [(0, 0), (1, 64), BEHIND, (16, 16)]
    try:
        reset(gm)
        gm.set_patterns(pats)
        gm.load_arena(K.HostArena.from_payloads(payloads))
        want = MM.oracle_counts(oracle, payloads, pats)
        assert gm.scan()[0].tolist() == want
        gm.set_windows(windows)
        gm.set_rules([([0], [1])])
        assert gm.scan()[0].tolist() == want                           # kmpgpu_scan does not look at windows
        gm.scan_enqueue()
        assert gm.counts_read().tolist() == want                       # nor does kmpgpu_scan_enqueue
        gm.set_option(OPT_ACCUMULATE, 1)
        gm.counts_reset()
        gm.scan_enqueue(); gm.scan_enqueue()
        st = MM.starts(payloads, pats, windows)
        recs, hits = MM.records(st), MM.hits(st)
        check_offsets(gm, recs, want)
        check_packets(gm, hits, want)
        check_rules(gm, hits, gm.rules, want)
        assert gm.counts_read().tolist() == [2 * c for c in want]
        gm.set_option(OPT_ACCUMULATE, 0)
        # pkt_counts[i] == 0 no longer implies counts[i] == 0
        assert hits[2].sum() == 0 and want[2] > 0
    finally:
        reset(gm)


# ------------------------------------------------------------------------------------------------
# 6. life cycle and errors
# ------------------------------------------------------------------------------------------------
def test_life_cycle_and_errors(gm, oracle):
    rng = random.Random("errors")
    plant = [b"abc", b"dA", b"b"]
    payloads = make_payloads(rng, "mixed", plant, n=150)
    pats = list(plant)
    g = _lib.gpu_lib()
    P = _lib.GPU_API["kmpgpu_set_windows"][1][1]

    def arr(v):
        return np.array(v, dtype=np.uint32)

    def call(ctx, first, last, n):
        a, b = arr(first), arr(last)
        return g.kmpgpu_set_windows(ctx, a.ctypes.data_as(P), b.ctypes.data_as(P), n)

    try:
        reset(gm)
        with GpuMatcher(0) as fresh:
            assert call(fresh._ctx, [0], [0], 1) == -3                 # KMPGPU_ESTATE: no patterns set
            assert g.kmpgpu_set_windows(fresh._ctx, None, None, 0) == -3
        gm.set_patterns(pats)
        gm.load_arena(K.HostArena.from_payloads(payloads))
        windows = [(0, 0), (3, 900), (16, None)]
        gm.set_windows(windows)
        st, free = MM.starts(payloads, pats, windows), MM.starts(payloads, pats)
        recs, hits = MM.records(st), MM.hits(st)
        counts = MM.oracle_counts(oracle, payloads, pats)
        assert recs != MM.records(free)
        # every refused call leaves the windows set before in force
        bad = [([0, 0], [1, 1], 2),                                    # n_pat differs from the context's
               ([0, 0, 0, 0], [1, 1, 1, 1], 4),
               ([0, 5, 0], [0, 4, 9], 3),                              # first > last
               ([1, 0, 0], [0, U32_MAX, U32_MAX], 3)]
        for first, last, n in bad:
            assert call(gm._ctx, first, last, n) == -2, (first, last, n)       # KMPGPU_EINVAL
            assert b"kmpgpu_set_windows" in g.kmpgpu_last_error()
            check_offsets(gm, recs, counts)
            check_packets(gm, hits, counts)
        assert g.kmpgpu_set_windows(gm._ctx, None, None, 3) == -2
        check_packets(gm, hits, counts)
        with pytest.raises(Exception):
            gm.set_windows([(0, 0)])
        assert gm.windows == windows
        check_packets(gm, hits, counts)
        # rules set before the windows see the windows' hits
        gm.set_rules([([0], [1]), ([2], [])])
        check_rules(gm, hits, gm.rules, counts)
        # n_pkts == 0: zeros, nothing launched
        gm.load_arena(np.zeros(64, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint32))
        res = gm.scan_packets(hits=True)
        assert res["pkt_counts"].tolist() == [0] * 3 and res["counts"].tolist() == [0] * 3 and res["timing"].launches == 0
        res = gm.scan_rules(hits=True)
        assert res["rule_pkt_counts"].tolist() == [0, 0] and res["hits"].shape == (2, 0)
        got, found, cnt = gm.scan_offsets(16)
        assert found == 0 and len(got) == 0 and cnt.tolist() == [0] * 3
        # set_patterns drops the windows
        gm.load_arena(K.HostArena.from_payloads(payloads))
        check_packets(gm, hits, counts)
        gm.set_patterns(pats)
        assert gm.windows == []
        check_offsets(gm, MM.records(free), counts)
        check_packets(gm, MM.hits(free), counts)
    finally:
        reset(gm)


# ------------------------------------------------------------------------------------------------
# 7. the command lines: KMPGPU_WINDOWS_FILE
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prog,extra", [("serial", []), ("openmp_data", ["2"])])
def test_cli_windows_file(tokens, tmp_path, prog, extra):
    arena = K.HostArena.from_pcap(os.path.join(DATA, "udp_1000.pcap"), "udp")
    payloads = [bytes(arena.payload(k)) for k in range(arena.n_pkts)]
    free = MM.starts(payloads, tokens)
    free_recs, free_hits = MM.records(free), MM.hits(free)
    # a window on the patterns that hit most: anchored, a range, an open end, one behind everything
    busy = [int(i) for i in np.argsort(-free_hits.sum(axis=1))[:8]]
    kinds = [(0, 0), (0, 63), (16, None), (1, 200), BEHIND, (0, 15), (32, 1024), (0, None)]
    windows = [(0, None)] * len(tokens)
    text = "# pattern first last\n\n"
    for i, (a, b) in zip(busy, kinds):
        windows[i] = (a, b)
        text += f"{i} {a} {'*' if b is None else b}\n"
    wf = tmp_path / "windows.txt"
    wf.write_text(text)
    rules = [([busy[0]], []), ([busy[1]], [busy[2]]), ([busy[3], busy[5]], []), ([], [busy[7]])]
    rf = tmp_path / "rules.txt"
    rf.write_text("".join(" ".join([str(i) for i in pos] + [f"!{i}" for i in neg]) + "\n" for pos, neg in rules))
    st = MM.starts(payloads, tokens, windows)
    recs, hits = MM.records(st), MM.hits(st)
    assert 0 < len(recs) < len(free_recs)
    off, pk, al = tmp_path / "offsets.csv", tmp_path / "packets.csv", tmp_path / "alerts.csv"
    r = run_cli(prog, extra=extra, env_extra={"KMPGPU_WINDOWS_FILE": str(wf), "KMPGPU_OFFSETS_FILE": str(off), "KMPGPU_PACKETS_FILE": str(pk),
                                              "KMPGPU_RULES_FILE": str(rf), "KMPGPU_ALERTS_FILE": str(al)})
    assert r.returncode == 0, r.stderr
    with open(os.path.join(GOLDEN, "stdout_udp_1000_udp.txt")) as f:
        assert strip_elapsed(r.stdout) == f.read()                                  # the counts do not follow the windows
    got = sorted(tuple(int(x) for x in line.split(",")) for line in off.read_text().splitlines())
    assert got == sorted(recs)
    got = [tuple(int(x) for x in line.split(",")) for line in pk.read_text().splitlines()]
    assert got == sorted((int(k), int(i)) for i, k in np.argwhere(hits))
    got = [tuple(int(x) for x in line.split(",")) for line in al.read_text().splitlines()]
    assert got == sorted((int(k), int(r_)) for r_, k in np.argwhere(MM.rule_rows(hits, rules)))
    # a windows file that does not parse, or one without an output file that it could act on: exit 1
    bad = tmp_path / "bad.txt"
    bad.write_text(f"{busy[0]} 0 0\n{busy[1]} 9 3\n")
    r = run_cli(prog, extra=extra, env_extra={"KMPGPU_WINDOWS_FILE": str(bad), "KMPGPU_PACKETS_FILE": str(pk)})
    assert r.returncode == 1 and "line 2: " in r.stderr and r.stdout == ""
    r = run_cli(prog, extra=extra, env_extra={"KMPGPU_WINDOWS_FILE": str(tmp_path / "none.txt"), "KMPGPU_PACKETS_FILE": str(pk)})
    assert r.returncode == 1 and r.stdout == ""
    r = run_cli(prog, extra=extra, env_extra={"KMPGPU_WINDOWS_FILE": str(wf)})
    assert r.returncode == 1 and "no effect" in r.stderr and r.stdout == ""
