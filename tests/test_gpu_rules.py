"""Content rules (kmpgpu_set_rules, kmpgpu_scan_rules, GpuMatcher.set_rules / scan_rules) on a real MI355X.

The expectation is the host model of tests/match_model.py: the rules are applied to its hit matrix with numpy, and the pattern
totals are the model's own counts.  Nothing of it comes from the library.  Every output of the call is compared exactly, through
the C-ABI and as whole words, so that a bit behind n_pkts shows.

The thresholds of the kernel as built (csrc/kmp_rules.hip) and the tests that cross them:
  * a group of cl = 1, 2, 4 .. 64 lanes covers a rule's row, two words per lane, cl the smallest power of two with
    2 cl >= W: the group size steps at 128 * {1, 2, 4 .. 64} payloads, the widest group and a block's column span (2 * 64
    words) end at 8192 payloads -- test_column_edges, n_pkts = 128 * 2^j - 1 and + 1 up to 8193 (two blocks in x);
  * W odd (a padding word per row on the device) and even, the last word full or not -- test_column_edges, 1 .. 129;
  * a block takes 256 / cl rules per round: 256 at 100 payloads -- test_row_edges, 255 / 256 / 257 rules;
  * the grid has at most 1024 blocks in y, further rules go in further rounds of the grid: 4 * 1024 rules at 8193
    payloads -- test_row_edges, 4100 rules x 8193 payloads; 70 000 rules x 100 payloads is past any 65 535 limit;
  * a rule's head carries two terms (two row loads in flight), every further quad four: test_term_counts, 1 .. 11 terms
    (one below / at / above 2, 2 + 4 and 2 + 8) and 100;
  * a lane stops reading a rule's quads when its accumulator is empty: the rules of test_term_counts whose deciding term
    comes last, positive and negated.

Run on a real MI355X:  python -m pytest tests/test_gpu_rules.py -m gpu
"""
import os
import random
import subprocess

import numpy as np
import pytest

from conftest import DATA, GOLDEN

pytestmark = pytest.mark.gpu

from gpu_support import KERNELS, gm, load, reset, run_cli, strip_elapsed  # noqa: E402,F401  (torch first)

import match_model as MM  # noqa: E402
import multithreading_string_matching_amd as K  # noqa: E402
from match_model import RULE_NOT as NOT  # noqa: E402
from multithreading_string_matching_amd import _lib  # noqa: E402
from multithreading_string_matching_amd.matcher import (  # noqa: E402
    KERNEL_GENERAL, MODE_AUTOMATON, OPT_ACCUMULATE, OPT_FUSED, OPT_KERNEL, OPT_MODE, OPT_REPACK, OPT_WHOLE_PAYLOAD, GpuMatcher)

EINVAL, ESTATE = -2, -3
ALPHABET = b"abcdAB"
SENTINEL = 0xA5A5A5A5A5A5A5A5                          # what the output buffers hold before a call


def scan_raw(gm, n_rules, skip=()):
    """kmpgpu_scan_rules through the C-ABI into buffers full of SENTINEL; skip: outputs passed as NULL.
    Returns (rc, {name: array})."""
    n_pkts, _ = gm.arena_info()
    W = (n_pkts + 63) // 64
    bufs = {"rule_pkt_counts": np.full(n_rules + 1, SENTINEL, dtype=np.uint64), "any": np.full(W + 1, SENTINEL, dtype=np.uint64),
            "hits": np.full(n_rules * W + 1, SENTINEL, dtype=np.uint64), "counts": np.full(len(gm.patterns) + 1, SENTINEL, dtype=np.uint64)}
    args = [None if k in skip else bufs[k].ctypes.data for k in ("rule_pkt_counts", "any", "hits", "counts")]
    t = _lib.Timing()
    rc = _lib.gpu_lib().kmpgpu_scan_rules(gm._ctx, *args, t)
    bufs["timing"] = t
    return rc, bufs


def check(gm, hits, counts, rules, skip=()):
    """one kmpgpu_scan_rules against the model: every word of every output, and nothing written behind them"""
    want = MM.rule_rows(hits, rules)
    n_rules, n_pkts = want.shape
    W = (n_pkts + 63) // 64
    rc, got = scan_raw(gm, n_rules, skip)
    assert rc == 0, _lib.gpu_lib().kmpgpu_last_error()
    expect = {"rule_pkt_counts": want.sum(axis=1).astype(np.uint64), "any": MM.words(want.any(axis=0)) if n_rules else np.zeros(W, np.uint64),
              "hits": MM.words(want).reshape(-1), "counts": np.array(counts, dtype=np.uint64)}
    for name, e in expect.items():
        g = got[name]
        assert g[-1] == SENTINEL, name                                        # nothing behind the output
        if name in skip:
            assert (g == SENTINEL).all(), name
            continue
        bad = np.flatnonzero(g[:-1] != e)
        assert bad.size == 0, (name, [(int(j), hex(int(g[j])), hex(int(e[j]))) for j in bad[:6]])
    return got


POOL_PATS = [b"ab", b"cdA", b"B", b"abcd", b"dd", b"aBc", b"ba", b"AB", b"cab", b"dAb"]


def small_payloads(rng, n, plant, max_len=64, nul=0.0):
    """payloads of 0..max_len bytes over ALPHABET with planted patterns: most patterns hit some payloads and miss others"""
    out = []
    for _ in range(n):
        L = rng.randrange(0, max_len + 1)
        b = bytearray(rng.choice(ALPHABET) for _ in range(L))
        for _ in range(rng.randrange(0, 3)):
            p = rng.choice(plant)
            if len(p) <= L:
                s = rng.randrange(L - len(p) + 1)
                b[s:s + len(p)] = p
        if nul and L and rng.random() < nul:
            b[rng.randrange(L)] = 0
        out.append(bytes(b))
    return out


@pytest.fixture(scope="module")
def pool():
    """8193 small payloads x POOL_PATS and their host model, computed once: the edge tests take prefixes of it"""
    rng = random.Random(8193)
    payloads = small_payloads(rng, 8193, POOL_PATS)
    per_payload = MM.per_payload(MM.starts(payloads, POOL_PATS))
    hits = per_payload > 0
    assert all(0 < h.sum() < len(payloads) for h in hits)                     # every pattern hits some payloads and misses others
    return payloads, hits, np.cumsum(per_payload, axis=1)


def pool_prefix(pool, n):
    payloads, hits, cum = pool
    return payloads[:n], hits[:, :n], [int(x) for x in cum[:, n - 1]]


def short_rules(rng, n_rules, n_pat):
    """one- and two-term rules, about a third of the terms negated"""
    rules = []
    for _ in range(n_rules):
        pos, neg = [], []
        for _ in range(rng.randrange(1, 3)):
            (neg if rng.random() < 0.35 else pos).append(rng.randrange(n_pat))
        rules.append((pos, neg))
    return rules


# ------------------------------------------------------------------------------------------------
# 1. column edges
# ------------------------------------------------------------------------------------------------
EDGE_RULES = [([], [0, 2, 4]),                # all negated: the tail mask
              ([], [5]),
              ([0], []), ([1, 2], []), ([0], [2]), ([3], [3]), ([2, 2], [1, 1]), ([0], [2]), ([6, 8, 0], [9, 4, 7])]
COLUMN_EDGES = [1, 63, 64, 65, 127, 128, 129] + [128 * (1 << j) + d for j in range(1, 7) for d in (-1, 1)] + [8192]


@pytest.mark.parametrize("n_pkts", COLUMN_EDGES)
def test_column_edges(gm, pool, n_pkts):
    payloads, hits, counts = pool_prefix(pool, n_pkts)
    reset(gm)
    gm.set_patterns(POOL_PATS)
    gm.set_rules(EDGE_RULES)
    gm.load_arena(K.HostArena.from_payloads(payloads))
    got = check(gm, hits, counts, EDGE_RULES)
    # an all-negated rule matches every payload that holds none of its patterns, the empty ones included
    empty = np.array([len(t) == 0 for t in payloads])
    want = MM.rule_rows(hits, EDGE_RULES)
    assert (want[0][empty]).all() and int(got["rule_pkt_counts"][0]) == int((~(hits[0] | hits[2] | hits[4])).sum())
    assert int(got["rule_pkt_counts"][5]) == 0                                 # i and !i never matches
    # the Python view of the same call
    res = gm.scan_rules(hits=True)
    assert np.array_equal(res["hits"], want) and res["any"].tolist() == want.any(axis=0).tolist()
    assert res["rule_pkt_counts"].tolist() == want.sum(axis=1).tolist() and res["counts"].tolist() == counts
    assert res["timing"].launches >= 2                                         # a scan launch and the rules kernel


# ------------------------------------------------------------------------------------------------
# 2. row edges
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rules, n_pkts", [(1, 100), (255, 100), (256, 100), (257, 100), (3000, 100), (70000, 100), (4100, 8193)])
def test_row_edges(gm, pool, n_rules, n_pkts):
    payloads, hits, counts = pool_prefix(pool, n_pkts)
    rng = random.Random(n_rules)
    rules = short_rules(rng, n_rules, len(POOL_PATS))
    rules[-1] = ([], [1, 3])                                                   # the last row: all negated
    reset(gm)
    gm.set_patterns(POOL_PATS)
    gm.set_rules(rules)
    gm.load_arena(K.HostArena.from_payloads(payloads))
    got = check(gm, hits, counts, rules)
    assert got["rule_pkt_counts"][:-1].any()


# ------------------------------------------------------------------------------------------------
# 3. term counts
# ------------------------------------------------------------------------------------------------
def test_term_counts(gm, pool):
    n_pkts = 1000
    payloads, hits, counts = pool_prefix(pool, n_pkts)
    # patterns 10 .. 12 repeat 0, 2 and 5: rules over duplicate patterns
    pats = POOL_PATS + [POOL_PATS[0], POOL_PATS[2], POOL_PATS[5]]
    hits = np.concatenate([hits, hits[[0, 2, 5]]])
    counts = counts + [counts[0], counts[2], counts[5]]
    rng = random.Random(11)
    rules = []
    for k in list(range(1, 12)) + [100]:
        rules.append(([0] * (k - 1) + [2], []))                                # the deciding term comes last: positive ...
        rules.append(([0] * (k - 1), [2]))                                     # ... and negated
        rules.append(([], [1] * (k - 1) + [4]))
        rules.append(([2] * k, []))                                            # one term, k times
        few = rng.sample(range(len(pats)), 3)
        picks = [rng.choice(few) for _ in range(k)]
        rules.append((picks[::2], picks[1::2]))                                # repeats, now and then i with !i
    rules += [([3], [3]), ([0, 1], [1]), ([0], []), ([0], []), ([10], []), ([0], [10]), ([12, 5], []), ([2], [11]), ([], [0, 10])]
    reset(gm)
    gm.set_patterns(pats)
    gm.set_rules(rules)
    gm.load_arena(K.HostArena.from_payloads(payloads))
    got = check(gm, hits, counts, rules)
    rc = got["rule_pkt_counts"]
    base = 12 * 5
    assert rc[base] == 0 and rc[base + 1] == 0                                 # i with !i
    assert rc[base + 2] == rc[base + 3] == rc[base + 4] == hits[0].sum()       # identical rules, a duplicate pattern
    assert rc[base + 5] == 0 and rc[base + 7] == 0                             # a pattern and not its duplicate
    W = (n_pkts + 63) // 64
    rows = got["hits"][:-1].reshape(len(rules), W)
    assert np.array_equal(rows[base + 2], rows[base + 3]) and np.array_equal(rows[base + 2], rows[base + 4])


# ------------------------------------------------------------------------------------------------
# 4. every way a pass is made
# ------------------------------------------------------------------------------------------------
MIXED_PATS = [b"ab", b"cdA", b"B", b"aBcd", b"DD", b"abc", b"ba", b"Ab", b"cab", b"d"]
MIXED_NOCASE = [False, True, False, True, True, False, True, True, False, False]
MIXED_RULES = [([0], []), ([1, 2], []), ([3], [4]), ([], [0, 4, 9]), ([5, 6], [7]), ([8], [8]), ([1], [2, 3]), ([9, 0], []), ([], [7])]


def _pass_arena(rng, kind):
    """(payloads, slot bytes or None)"""
    if kind == "uniform":
        payloads = []
        for _ in range(300):
            b = bytearray(rng.choice(ALPHABET) for _ in range(512))
            for _ in range(3):
                p = rng.choice(MIXED_PATS)
                s = rng.randrange(512 - len(p) + 1)
                b[s:s + len(p)] = p
            payloads.append(bytes(b[:12]) + b"e" * 488 + bytes(b[500:]))       # mostly filler: the patterns stay selective
        return payloads, None
    if kind == "empty":
        payloads = [b"" if rng.random() < 0.5 else t for t in small_payloads(rng, 700, MIXED_PATS)]
        return payloads, None
    payloads = small_payloads(rng, 700, MIXED_PATS, max_len=64 if kind == "dirty" else 300)
    if kind != "dirty":
        return payloads, None
    slots = []
    for t in payloads:                                   # the padding goes on with text that would complete or add a match
        pad = (-len(t)) % 16 or (16 if not t else 0)
        p = rng.choice(MIXED_PATS)
        slots.append(t + (p * (pad // len(p) + 1))[:pad])
    return payloads, slots


@pytest.mark.parametrize("kind", ["uniform", "mixed", "empty", "dirty"])
def test_every_pass(gm, kind):
    rng = random.Random(f"rules-{kind}")
    payloads, slots = _pass_arena(rng, kind)
    st = MM.starts(payloads, MIXED_PATS, nocase=MIXED_NOCASE)
    hits, counts = MM.hits(st), MM.counts(st)
    assert (hits.sum(axis=1) > 0).all()
    keep = None
    try:
        reset(gm)
        gm.set_patterns(MIXED_PATS, nocase=MIXED_NOCASE)
        gm.set_rules(MIXED_RULES)
        keep = load(gm, payloads, slots)
        for name, kernel, fused in KERNELS:
            gm.set_option(OPT_KERNEL, kernel); gm.set_option(OPT_FUSED, fused)
            check(gm, hits, counts, MIXED_RULES)
    finally:
        reset(gm)
        del keep


def test_arena_kept_in_place(gm):
    """OPT_REPACK = 0 with slots not back to back: the call packs the arena once, as kmpgpu_scan_packets does."""
    rng = random.Random(77)
    payloads = small_payloads(rng, 500, MIXED_PATS, max_len=200)
    ln = np.array([len(t) for t in payloads], dtype=np.uint32)
    slot = np.maximum(16, (ln.astype(np.uint64) + 15) // 16 * 16) + 32           # gaps between the slots
    order = list(range(len(payloads)))
    rng.shuffle(order)                                                            # slots not in payload order
    off = np.zeros(len(payloads), dtype=np.uint64)
    pos = 0
    for k in order:
        off[k] = pos
        pos += int(slot[k])
    arena = np.zeros(pos + 64, dtype=np.uint8)
    for k, t in enumerate(payloads):
        arena[int(off[k]):int(off[k]) + len(t)] = np.frombuffer(t, dtype=np.uint8)
    st = MM.starts(payloads, MIXED_PATS, nocase=MIXED_NOCASE)
    hits, counts = MM.hits(st), MM.counts(st)
    try:
        reset(gm)
        gm.set_option(OPT_REPACK, 0)
        gm.set_patterns(MIXED_PATS, nocase=MIXED_NOCASE)
        gm.set_rules(MIXED_RULES)
        gm.load_arena(arena, off, ln)
        assert gm.scan()[0].tolist() == counts
        check(gm, hits, counts, MIXED_RULES)
        check(gm, hits, counts, MIXED_RULES)
        assert gm.scan()[0].tolist() == counts
    finally:
        reset(gm)


def test_whole_payload_switched_between_calls(gm):
    rng = random.Random(9)
    payloads = small_payloads(rng, 900, MIXED_PATS, nul=0.6)
    st = {w: MM.starts(payloads, MIXED_PATS, nocase=MIXED_NOCASE, whole=bool(w)) for w in (0, 1)}
    model = {w: (MM.hits(st[w]), MM.counts(st[w])) for w in (0, 1)}
    assert not np.array_equal(MM.rule_rows(model[0][0], MIXED_RULES), MM.rule_rows(model[1][0], MIXED_RULES))
    try:
        reset(gm)
        gm.set_patterns(MIXED_PATS, nocase=MIXED_NOCASE)
        gm.set_rules(MIXED_RULES)
        gm.load_arena(K.HostArena.from_payloads(payloads))
        for w in (0, 1, 0, 1):                           # nothing reloaded, re-attached or re-set in between
            gm.set_option(OPT_WHOLE_PAYLOAD, w)
            check(gm, model[w][0], model[w][1], MIXED_RULES)
    finally:
        reset(gm)


# ------------------------------------------------------------------------------------------------
# 5. context state
# ------------------------------------------------------------------------------------------------
def test_state(gm, pool):
    g = _lib.gpu_lib()
    big, big_hits, big_counts = pool_prefix(pool, 5000)
    small, small_hits, small_counts = pool_prefix(pool, 70)
    rules = EDGE_RULES
    off, terms = MM.flat_rules(rules)

    def set_raw(ctx, off, terms, n):
        return g.kmpgpu_set_rules(ctx, off.ctypes.data_as(_lib.u32p), terms.ctypes.data_as(_lib.u32p), n)

    try:
        reset(gm)
        with GpuMatcher(0) as fresh:
            assert set_raw(fresh._ctx, off, terms, len(rules)) == ESTATE           # rules before patterns
            assert g.kmpgpu_scan_rules(fresh._ctx, None, None, None, None, None) == ESTATE
            fresh.set_patterns(POOL_PATS)
            fresh.load_arena(K.HostArena.from_payloads(small))
            assert g.kmpgpu_scan_rules(fresh._ctx, None, None, None, None, None) == ESTATE   # patterns and arena, no rules
        gm.set_patterns(POOL_PATS)
        gm.load_arena(K.HostArena.from_payloads(big))
        gm.set_rules(rules)
        check(gm, big_hits, big_counts, rules)
        # every EINVAL leaves the rules set before in force
        bad = [(np.array([1, 2], np.uint32), np.array([0, 1], np.uint32), 1),                    # rule_off[0] != 0
               (np.array([0, 2, 1], np.uint32), np.array([0, 1], np.uint32), 2),                 # decreasing
               (np.array([0, 1, 1], np.uint32), np.array([0], np.uint32), 2),                    # a rule without terms
               (np.array([0, 2], np.uint32), np.array([0, len(POOL_PATS)], np.uint32), 1),       # index >= n_pat
               (np.array([0, 1], np.uint32), np.array([len(POOL_PATS) | NOT], np.uint32), 1)]    # ... negated
        for o, t, n in bad:
            assert set_raw(gm._ctx, o, t, n) == EINVAL
            check(gm, big_hits, big_counts, rules)
        with pytest.raises(K.KmpGpuError):
            gm.set_rules([([len(POOL_PATS)], [])])
        assert gm.rules == rules
        # streaming kernels only
        for key, val in ((OPT_MODE, MODE_AUTOMATON), (OPT_KERNEL, KERNEL_GENERAL)):
            gm.set_option(key, val)
            assert g.kmpgpu_scan_rules(gm._ctx, None, None, None, None, None) == EINVAL
            reset(gm)
        # each output in turn as NULL, and all of them
        for name in ("rule_pkt_counts", "any", "hits", "counts"):
            check(gm, big_hits, big_counts, rules, skip=(name,))
        check(gm, big_hits, big_counts, rules, skip=("rule_pkt_counts", "any", "hits", "counts"))
        # scan_packets before and after scan_rules: identical
        before = gm.scan_packets(hits=True)
        check(gm, big_hits, big_counts, rules)
        after = gm.scan_packets(hits=True)
        for name in ("pkt_counts", "any", "hits", "counts"):
            assert np.array_equal(before[name], after[name]), name
        assert np.array_equal(before["hits"], big_hits) and before["counts"].tolist() == big_counts
        # the context's counters under OPT_ACCUMULATE are left alone
        gm.set_option(OPT_ACCUMULATE, 1)
        gm.counts_reset()
        gm.scan_enqueue(); gm.scan_enqueue()
        assert gm.counts_read().tolist() == [2 * c for c in big_counts]
        check(gm, big_hits, big_counts, rules)
        assert gm.counts_read().tolist() == [2 * c for c in big_counts]
        gm.set_option(OPT_ACCUMULATE, 0)
        assert gm.scan()[0].tolist() == big_counts
        # a small arena after a large one: no stale bits, no stale totals
        gm.load_arena(K.HostArena.from_payloads(small))
        check(gm, small_hits, small_counts, rules)
        # n_pkts == 0: zeros, nothing launched
        gm.load_arena(np.zeros(64, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint32))
        rc, got = scan_raw(gm, len(rules))
        assert rc == 0 and got["timing"].launches == 0
        assert not got["rule_pkt_counts"][:-1].any() and not got["counts"][:-1].any()
        assert got["any"][0] == SENTINEL and got["hits"][0] == SENTINEL              # W == 0: no words
        res = gm.scan_rules(hits=True)
        assert res["hits"].shape == (len(rules), 0) and res["any"].size == 0 and res["rule_pkt_counts"].tolist() == [0] * len(rules)
        gm.load_arena(K.HostArena.from_payloads(small))
        check(gm, small_hits, small_counts, rules)
        # n_rules == 0 clears the rules; new patterns drop them
        gm.set_rules([])
        assert g.kmpgpu_scan_rules(gm._ctx, None, None, None, None, None) == ESTATE
        gm.set_rules(rules)
        check(gm, small_hits, small_counts, rules)
        gm.set_patterns(POOL_PATS)
        assert gm.rules == []
        assert g.kmpgpu_scan_rules(gm._ctx, None, None, None, None, None) == ESTATE
        assert np.array_equal(gm.scan_packets(hits=True)["hits"], small_hits)
    finally:
        reset(gm)


# ------------------------------------------------------------------------------------------------
# 6. the capture fixture x strings.txt
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def udp1000(tokens):
    """udp_1000.pcap x the 97 tokens: payloads, host hit matrix, totals, 40 generated rules and their rows"""
    arena = K.HostArena.from_pcap(os.path.join(DATA, "udp_1000.pcap"), "udp")
    payloads = [arena.payload(k) for k in range(arena.n_pkts)]
    st = MM.starts(payloads, tokens)
    hits, counts = MM.hits(st), MM.counts(st)
    rng = random.Random(1000)
    live = [i for i in range(len(tokens)) if hits[i].any()]
    rules = []
    for _ in range(40):
        pos = [rng.choice(live) if rng.random() < 0.8 else rng.randrange(len(tokens)) for _ in range(rng.randrange(0, 4))]
        neg = [rng.choice(live) if rng.random() < 0.6 else rng.randrange(len(tokens)) for _ in range(rng.randrange(0 if pos else 1, 3))]
        rules.append((pos, neg))
    want = MM.rule_rows(hits, rules)
    assert want.any() and not want.all()
    return arena, hits, counts, rules, want


@pytest.mark.parametrize("route", ["load_arena", "load_pcap_frames"])
def test_fixture(gm, tokens, fixture_counts, udp1000, route):
    arena, hits, counts, rules, _ = udp1000
    assert counts == fixture_counts["fixtures"]["udp_1000.pcap:udp"]["counts"]
    reset(gm)
    gm.set_patterns(tokens)
    gm.set_rules(rules)
    if route == "load_arena":
        gm.load_arena(arena)
    else:
        n, _ = gm.load_pcap_frames(os.path.join(DATA, "udp_1000.pcap"), "udp")
        assert n == arena.n_pkts
    check(gm, hits, counts, rules)


# ------------------------------------------------------------------------------------------------
# 7. the command lines: KMPGPU_RULES_FILE + KMPGPU_ALERTS_FILE
# ------------------------------------------------------------------------------------------------
def _rules_file(path, rules):
    lines = ["# generated", ""]
    for pos, neg in rules:
        lines.append(" ".join([str(i) for i in pos] + [f"!{i}" for i in neg]))
    path.write_text("\n".join(lines) + "\n")


CLI_RUNS = [("serial", []), ("openmp_data", ["1"]), ("openmp_data", ["3"])]


@pytest.mark.parametrize("with_packets", [False, True])
@pytest.mark.parametrize("run", CLI_RUNS, ids=["serial", "openmp_data-1", "openmp_data-3"])
def test_cli_alerts_file(udp1000, tmp_path, run, with_packets):
    prog, extra = run
    _, hits, _, rules, want = udp1000
    golden = open(os.path.join(GOLDEN, "stdout_udp_1000_udp.txt")).read()
    _rules_file(tmp_path / "rules.txt", rules)
    alerts, packets = tmp_path / "alerts.csv", tmp_path / "packets.csv"
    env = {"KMPGPU_RULES_FILE": str(tmp_path / "rules.txt"), "KMPGPU_ALERTS_FILE": str(alerts)}
    if with_packets:
        env["KMPGPU_PACKETS_FILE"] = str(packets)
    r = run_cli(prog, extra=extra, env_extra=env, scrub=None)
    assert r.returncode == 0, r.stderr
    assert strip_elapsed(r.stdout) == golden
    got = [tuple(int(x) for x in line.split(",")) for line in alerts.read_text().splitlines()]
    assert got == sorted((int(k), int(i)) for i, k in np.argwhere(want))      # sorted by payload, then by rule, as written
    if with_packets:
        # the packets file is what it is without rules: the model's (payload, pattern) pairs
        pk = [tuple(int(x) for x in line.split(",")) for line in packets.read_text().splitlines()]
        assert pk == sorted((int(k), int(i)) for i, k in np.argwhere(hits))


@pytest.mark.parametrize("which", ["KMPGPU_RULES_FILE", "KMPGPU_ALERTS_FILE", "parse"])
def test_cli_rules_errors(udp1000, tmp_path, which):
    _, _, _, rules, _ = udp1000
    _rules_file(tmp_path / "rules.txt", rules)
    env = {k: v for k, v in os.environ.items() if k not in ("KMPGPU_RULES_FILE", "KMPGPU_ALERTS_FILE")}
    if which == "parse":
        (tmp_path / "rules.txt").write_text("0 1\n2 97\n")                     # strings.txt has 97 tokens: index 97 is one too far
        env.update(KMPGPU_RULES_FILE=str(tmp_path / "rules.txt"), KMPGPU_ALERTS_FILE=str(tmp_path / "alerts.csv"))
    else:
        env[which] = str(tmp_path / ("rules.txt" if which == "KMPGPU_RULES_FILE" else "alerts.csv"))
    r = subprocess.run([os.path.join(_lib.BINDIR, "serial"), os.path.join(DATA, "udp_1000.pcap"), os.path.join(DATA, "strings.txt"), "udp"],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 1 and r.stdout == "" and r.stderr.strip()
    assert not (tmp_path / "alerts.csv").exists()
    if which == "parse":
        assert "line 2: " in r.stderr
