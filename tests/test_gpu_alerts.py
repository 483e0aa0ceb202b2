"""kmpgpu_scan_alerts / kmpgpu_alerts_read on the GPU: the set bits of a row family as (payload, row) records, sorted by payload, then
row, against the rows of tests/match_model.py (and tests/chain_model.py).  The expected list is [(k, i) for k, i in
np.argwhere(rows.T)]; every comparison is exact and in order, never as a set.

What the new kernels (csrc/kmp_alerts.hip) and the scan behind them tile by, and the case that crosses each:
  A1  64 rows per transpose step                                          test_row_edges: 1, 63, 64, 65, 129 rows
  A2  64 payloads per column word, 4 words (256 payloads) per wavefront,
      16 words (1 024 payloads) per block; KMP_SCAN_TILE = 1 024
      payloads per block of kmp_scan_local_kernel                         test_payload_edges: 1 .. 2 049 payloads
  A3  KMP_ALERTS_BLOCKS = 1 024 blocks of 4 wavefronts of 4 words: the
      grid-stride loops of both kernels go round past 1 048 576 payloads;
      kmp_scan_totals_kernel takes 256 tiles per round: past 262 144      test_past_the_grid_cap: 1 048 576 + 321 payloads
  A4  a column word, and a whole wavefront's four, with any[] == 0        test_empty_words_between
"""
import ctypes as C
import os
import random

import numpy as np
import pytest

from conftest import DATA

pytestmark = pytest.mark.gpu

from gpu_support import KERNELS, gm, load, reset, run_cli  # noqa: E402,F401  (torch first)

import chain_model as CM  # noqa: E402
import match_model as MM  # noqa: E402
import multithreading_string_matching_amd as K  # noqa: E402
from multithreading_string_matching_amd import _lib  # noqa: E402
from multithreading_string_matching_amd.matcher import (  # noqa: E402
    ALERT_CHAINS, ALERT_DTYPE, ALERT_PATTERNS, ALERT_RELATIONS, ALERT_RULES, ALERTS_ALL, KERNEL_GENERAL, MODE_AUTOMATON, OPT_ACCUMULATE,
    OPT_FUSED, OPT_KERNEL, OPT_MODE, OPT_WHOLE_PAYLOAD, GpuMatcher)

EINVAL, ESTATE = -2, -3
KMP_ALERTS_BLOCKS, BLOCK_WAVES, ALERTS_WORDS = 1024, 4, 4          # csrc/kmp_alerts.hip, csrc/kmp_device.h
PAST_THE_CAP = KMP_ALERTS_BLOCKS * BLOCK_WAVES * ALERTS_WORDS * 64 + 321

# 16-byte payloads of four 4-byte fields: field i holds token i or dots, so the hit matrix of the first four patterns is what the test
# chooses.  The fifth pattern occurs nowhere: a rule of "not NEVER" matches every payload.
TOKENS = [b"AAAA", b"BBBB", b"CCCC", b"DDDD", b"ZZZZ"]
NEVER = 4


def arena16(hits):
    """hits: bool[4, n] -> (arena uint8[16 n + 64], off, len) of n 16-byte payloads that hold token i exactly where hits[i] says"""
    n = hits.shape[1]
    a = np.full((n, 16), ord("."), dtype=np.uint8)
    for i in range(4):
        a[hits[i], 4 * i:4 * i + 4] = TOKENS[i][0]
    arena = np.concatenate([a.reshape(-1), np.zeros(64, np.uint8)])
    return arena, np.arange(n, dtype=np.uint64) * 16, np.full(n, 16, dtype=np.uint32)


def load16(gm, hits):
    """loads arena16(hits); returns the model's hit matrix of TOKENS over it (5 rows) and the totals"""
    arena, off, ln = arena16(hits)
    gm.load_arena(arena, off, ln)
    n = hits.shape[1]
    st = MM.starts([arena[16 * k:16 * k + 16].tobytes() for k in range(n)], TOKENS)
    model = MM.hits(st, len(TOKENS))
    assert np.array_equal(model[:4], hits) and not model[NEVER].any()
    return model, MM.counts(st, len(TOKENS))


def expected(rows):
    return [(int(k), int(i)) for k, i in np.argwhere(rows.T)]


def pairs(alerts):
    assert alerts.dtype == ALERT_DTYPE and not alerts["reserved"].any()
    return list(zip(alerts["packet"].tolist(), alerts["index"].tolist()))


def check_alerts(gm, family, rows, counts=None, max_records=None):
    """one alerts pass against the model's rows: the list exactly and in order, and every small output"""
    want = expected(rows)
    res = gm.scan_alerts(family, max_records)
    kept = len(want) if max_records is None else min(len(want), max_records)
    assert res["n_found"] == len(want)
    got = pairs(res["alerts"])
    assert len(got) == kept
    assert got == want[:kept], [(a, b) for a, b in zip(got, want) if a != b][:6]
    assert all(k < rows.shape[1] for k, _ in got)
    assert res["n_packets"] == int(rows.any(axis=0).sum())
    assert res["pkt_counts"].tolist() == rows.sum(axis=1).tolist()
    if counts is not None:
        assert res["counts"].tolist() == list(counts)
    return res


def rules_of(n_rules):
    """n_rules rows from five patterns: every third matches every payload (all-negated over the pattern that never occurs), the others
    hit chosen payloads"""
    return [([], [NEVER]) if r % 3 == 0 else ([r % 4], [(r + 1) % 4] if r % 2 else []) for r in range(n_rules)]


def random_hits(seed, n, p):
    return np.random.default_rng(seed).random((4, n)) < p


# ------------------------------------------------------------------------------------------------
# 1. rows, payloads, the grid cap
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rules", [1, 63, 64, 65, 129])
def test_row_edges(gm, n_rules):
    try:
        reset(gm)
        gm.set_patterns(TOKENS)
        hits, counts = load16(gm, random_hits(n_rules, 200, 0.3))
        rules = rules_of(n_rules)
        gm.set_rules(rules)
        rows = MM.rule_rows(hits, rules)
        res = check_alerts(gm, "rules", rows, counts)
        assert res["n_found"] >= 200                           # rule 0 matches every payload
    finally:
        reset(gm)


@pytest.mark.parametrize("n_pkts", [1, 63, 64, 65, 127, 1023, 1024, 1025, 2049])
def test_payload_edges(gm, n_pkts):
    try:
        reset(gm)
        gm.set_patterns(TOKENS)
        h = random_hits(n_pkts, n_pkts, 0.3)
        h[:, -1] = True                                        # the last payload is in the list
        hits, counts = load16(gm, h)
        check_alerts(gm, "patterns", hits, counts)
        rules = rules_of(5)
        gm.set_rules(rules)
        check_alerts(gm, "rules", MM.rule_rows(hits, rules), counts)
    finally:
        reset(gm)


def test_past_the_grid_cap(gm):
    """A3: more payloads than one round of either grid and of the totals kernel.  One pattern; the expected list comes from the chosen
    bits, and the model confirms the arena on a sample of it"""
    n = PAST_THE_CAP
    rng = np.random.default_rng(7)
    h = np.zeros((4, n), dtype=bool)
    h[0, rng.choice(n, 3000, replace=False)] = True
    h[0, [0, n - 1]] = True
    arena, off, ln = arena16(h)
    sample = np.concatenate([np.flatnonzero(h[0])[:500], rng.choice(n, 500)])
    st = MM.starts([arena[16 * k:16 * k + 16].tobytes() for k in sample], TOKENS[:1])
    assert MM.hits(st)[0].tolist() == h[0, sample].tolist()
    try:
        reset(gm)
        gm.set_patterns(TOKENS[:1])
        gm.load_arena(arena, off, ln)
        res = gm.scan_alerts("patterns")
        want = np.flatnonzero(h[0])
        assert res["n_found"] == want.size == res["n_packets"] and res["pkt_counts"].tolist() == [want.size]
        assert np.array_equal(res["alerts"]["packet"], want.astype(np.uint64)) and not res["alerts"]["index"].any()
        assert res["counts"].tolist() == [want.size]
    finally:
        reset(gm)


# ------------------------------------------------------------------------------------------------
# 2. densities
# ------------------------------------------------------------------------------------------------
def test_no_bit_set(gm):
    try:
        reset(gm)
        gm.set_patterns(TOKENS)
        hits, counts = load16(gm, np.zeros((4, 300), dtype=bool))
        res = check_alerts(gm, "patterns", hits, counts)
        assert res["n_found"] == 0 and res["n_packets"] == 0 and res["alerts"].size == 0
        assert gm.alerts_read(0, 0).size == 0
        gm.set_rules([([0], []), ([1, 2], [])])
        assert check_alerts(gm, "rules", np.zeros((2, 300), dtype=bool), counts)["n_found"] == 0
    finally:
        reset(gm)


def test_every_bit_set(gm):
    """65 all-negated rules x 1 100 payloads, every third payload empty: every bit below n_pkts is set, none above gives a record"""
    n = 1100
    payloads = [b"" if k % 3 == 0 else b"AAAA....CCCC...." for k in range(n)]
    st = MM.starts(payloads, TOKENS)
    hits, counts = MM.hits(st), MM.counts(st)
    try:
        reset(gm)
        gm.set_patterns(TOKENS)
        load(gm, payloads)
        rules = [([], [NEVER])] * 65
        gm.set_rules(rules)
        rows = MM.rule_rows(hits, rules)
        assert rows.all() and n % 64
        res = check_alerts(gm, "rules", rows, counts)
        assert res["n_found"] == 65 * n and res["n_packets"] == n and int(res["alerts"]["packet"].max()) == n - 1
    finally:
        reset(gm)


@pytest.mark.parametrize("where", ["first", "last"])
def test_one_bit(gm, where):
    n, n_rules = 1025, 65
    h = np.zeros((4, n), dtype=bool)
    h[0, 0 if where == "first" else n - 1] = True
    try:
        reset(gm)
        gm.set_patterns(TOKENS)
        hits, counts = load16(gm, h)
        rules = [([1], [])] * n_rules
        rules[0 if where == "first" else n_rules - 1] = ([0], [])
        gm.set_rules(rules)
        res = check_alerts(gm, "rules", MM.rule_rows(hits, rules), counts)
        assert pairs(res["alerts"]) == [(0, 0) if where == "first" else (n - 1, n_rules - 1)]
    finally:
        reset(gm)


@pytest.mark.parametrize("p", [0.01, 0.5])
def test_random_density(gm, p):
    n = 1500
    try:
        reset(gm)
        gm.set_patterns(TOKENS)
        hits, counts = load16(gm, random_hits(int(p * 100), n, p))
        check_alerts(gm, "patterns", hits, counts)
        rules = [([r % 4], []) for r in range(70)]             # rows of the patterns' density
        gm.set_rules(rules)
        check_alerts(gm, "rules", MM.rule_rows(hits, rules), counts)
    finally:
        reset(gm)


def test_empty_words_between(gm):
    """A4: column word 1 empty between words 0 and 2 (inside one wavefront's four), and the four words 4 .. 7 of a wavefront empty between
    two that are not"""
    n = 64 * 12
    h = np.zeros((4, n), dtype=bool)
    for lo in (0, 128, 64 * 9):
        h[:, lo:lo + 64] = random_hits(lo, 64, 0.4)
        h[0, lo] = True
    try:
        reset(gm)
        gm.set_patterns(TOKENS)
        hits, counts = load16(gm, h)
        any_words = MM.words(hits.any(axis=0))
        assert any_words[0] and not any_words[1] and any_words[2] and not any_words[4:8].any() and any_words[9]
        check_alerts(gm, "patterns", hits, counts)
    finally:
        reset(gm)


# ------------------------------------------------------------------------------------------------
# 3. max_records and alerts_read
# ------------------------------------------------------------------------------------------------
def test_max_records_and_pieces(gm):
    g = _lib.gpu_lib()
    try:
        reset(gm)
        gm.set_patterns(TOKENS)
        hits, counts = load16(gm, random_hits(3, 700, 0.2))
        want = expected(hits)
        n = len(want)
        assert n > 100
        for cap in (0, 1, n - 1, n, n + 1, ALERTS_ALL):
            check_alerts(gm, "patterns", hits, counts, max_records=cap)
        # the records stay on the device and are read in pieces
        res = gm.scan_alerts("patterns", max_records=n - 5, read=False)
        kept = n - 5
        assert res["n_found"] == n and res["alerts"].size == 0
        for first, cnt in ((0, 1), (3, 7), (61, 67), (kept - 9, 9), (kept, 0), (0, 0), (0, kept)):
            assert pairs(gm.alerts_read(first, cnt)) == want[first:first + cnt]
        # a range that leaves the kept prefix: KMPGPU_EINVAL, and the list survives
        buf = np.zeros(n + 8, dtype=ALERT_DTYPE)
        for first, cnt in ((0, kept + 1), (kept, 1), (kept + 1, 0), (5, ALERTS_ALL), (ALERTS_ALL, 2)):
            assert g.kmpgpu_alerts_read(gm._ctx, buf.ctypes.data, first, cnt) == EINVAL
            assert pairs(gm.alerts_read(kept - 2, 2)) == want[kept - 2:kept]
    finally:
        reset(gm)


# ------------------------------------------------------------------------------------------------
# 4. the four families, every way a hit is defined
# ------------------------------------------------------------------------------------------------
FAM_PATS = [b"ab", b"cd", b"abc", b"Dab", b"b", b"cda"]
FAM_RELATIONS = [(0, 1, 0, 6), (1, 0, None, 2), (2, 2, -3, 40), (4, 5, 1, None)]
FAM_CHAINS = [(0, (1, 0, 8), (4, 0, None)), (1, (0, None, 10)), (3, (1, 0, 20), (0, -2, 30))]
FAM_WINDOWS = [(0, 20), (2, None), (0, None), (0, 0), (1, 30), (0, None)]
FAM_NOCASE = [False, True, False, True, False, True]


def family_payloads(seed, n=400, nul=0.0):
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        L = rng.randrange(0, 61)
        b = bytearray(rng.choice(b"abcdABCD") for _ in range(L))
        if nul and L and rng.random() < nul:
            b[rng.randrange(L)] = 0
        out.append(bytes(b))
    return out


def family_rules(n_pat, n_rel, n_chains):
    rel, ch = n_pat, n_pat + n_rel
    return [([0], []), ([rel], []), ([ch], [rel + 1]), ([1, ch + 1], []), ([], [rel + 2, ch + 2]), ([2, rel + 3], [5]), ([], [ch])]


def check_families(gm, payloads, windows=None, nocase=None, whole=False, slots=None, kernels=KERNELS):
    st = MM.starts(payloads, FAM_PATS, windows=windows, nocase=nocase, whole=whole)
    counts = MM.counts(MM.starts(payloads, FAM_PATS, nocase=nocase, whole=whole))             # every match, in window or not
    hits = MM.hits(st)
    rel_rows = MM.relation_rows(st, FAM_PATS, FAM_RELATIONS)
    chain_rows = CM.chain_rows(st, FAM_PATS, FAM_CHAINS)
    rules = family_rules(len(FAM_PATS), len(FAM_RELATIONS), len(FAM_CHAINS))
    rule_rows = MM.rule_rows(np.concatenate([hits, rel_rows, chain_rows]), rules)
    assert hits.any() and rel_rows.any() and chain_rows.any() and rule_rows.any()
    gm.set_option(OPT_WHOLE_PAYLOAD, int(whole))
    gm.set_patterns(FAM_PATS, nocase=nocase or False)
    gm.set_relations(FAM_RELATIONS)
    gm.set_chains(FAM_CHAINS)
    gm.set_rules(rules)
    gm.set_windows(windows)
    keep = load(gm, payloads, slots)
    for _, kernel, fused in kernels:
        gm.set_option(OPT_KERNEL, kernel)
        gm.set_option(OPT_FUSED, fused)
        for family, rows, sibling, name in (("patterns", hits, gm.scan_packets, "pkt_counts"), ("rules", rule_rows, gm.scan_rules, "rule_pkt_counts"),
                                            ("relations", rel_rows, gm.scan_relations, "rel_pkt_counts"), ("chains", chain_rows, gm.scan_chains, "chain_pkt_counts")):
            res = check_alerts(gm, family, rows, counts)
            sib = sibling()
            assert res["pkt_counts"].tolist() == sib[name].tolist() and res["counts"].tolist() == sib["counts"].tolist()
            assert res["n_packets"] == int(sib["any"].sum())
    del keep


@pytest.mark.parametrize("how", ["plain", "windows", "whole", "nocase", "all"])
def test_families(gm, how):
    payloads = family_payloads(f"families-{how}", nul=0.4 if how in ("whole", "all") else 0.0)
    try:
        reset(gm)
        check_families(gm, payloads, windows=FAM_WINDOWS if how in ("windows", "all") else None,
                       nocase=FAM_NOCASE if how in ("nocase", "all") else None, whole=how in ("whole", "all"))
    finally:
        reset(gm)                                            # (the next set_patterns drops the windows)


def test_families_on_a_borrowed_arena_with_dirty_padding(gm):
    rng = random.Random("dirty")
    payloads = family_payloads("families-dirty")
    slots = []
    for t in payloads:                                   # the padding goes on with text that would complete or add a match
        pad = (-len(t)) % 16 or (16 if not t else 0)
        p = rng.choice(FAM_PATS)
        slots.append(t + (p * (pad // len(p) + 1))[:pad])
    try:
        reset(gm)
        check_families(gm, payloads, slots=slots)
    finally:
        reset(gm)


# ------------------------------------------------------------------------------------------------
# 5. context state
# ------------------------------------------------------------------------------------------------
def scan_raw(gm, family, cap=ALERTS_ALL):
    found = C.c_uint64(12345)
    return _lib.gpu_lib().kmpgpu_scan_alerts(gm._ctx, family, cap, C.byref(found), None, None, None, None), int(found.value)


def test_state(gm):
    g = _lib.gpu_lib()
    buf = np.zeros(16, dtype=ALERT_DTYPE)
    big, small = random_hits(11, 3000, 0.4), random_hits(12, 70, 0.1)
    rules = rules_of(7)
    try:
        reset(gm)
        with GpuMatcher(0) as fresh:
            assert g.kmpgpu_alerts_read(fresh._ctx, buf.ctypes.data, 0, 0) == ESTATE              # no alerts pass yet
            for family in (ALERT_PATTERNS, ALERT_RULES, ALERT_RELATIONS, ALERT_CHAINS):
                assert scan_raw(fresh, family)[0] == ESTATE                                        # no patterns
            fresh.set_patterns(TOKENS)
            fresh.load_arena(*arena16(small))
            for family in (ALERT_RULES, ALERT_RELATIONS, ALERT_CHAINS):
                assert scan_raw(fresh, family)[0] == ESTATE                                        # nothing of the family set
            assert scan_raw(fresh, ALERT_PATTERNS) == (0, int(small.sum()))
            for family in (-1, 4, 1000):
                assert scan_raw(fresh, family)[0] == EINVAL
            assert g.kmpgpu_scan_alerts(fresh._ctx, ALERT_PATTERNS, ALERTS_ALL, None, None, None, None, None) == EINVAL
        gm.set_patterns(TOKENS)
        gm.set_rules(rules)
        # the same pass twice: the same list; a large arena, then a small one: no stale record
        hits, counts = load16(gm, big)
        rows = MM.rule_rows(hits, rules)
        first = check_alerts(gm, "rules", rows, counts)
        again = check_alerts(gm, "rules", rows, counts)
        assert first["alerts"].tobytes() == again["alerts"].tobytes()
        # scan_packets and scan_rules return the same before and after an alerts pass
        before = (gm.scan_packets(hits=True), gm.scan_rules(hits=True))
        check_alerts(gm, "patterns", hits, counts)
        check_alerts(gm, "rules", rows, counts, max_records=10)
        after = (gm.scan_packets(hits=True), gm.scan_rules(hits=True))
        for b, a in zip(before, after):
            for key in b:
                if key != "timing":
                    assert np.array_equal(b[key], a[key]), key
        s_hits, s_counts = load16(gm, small)
        assert g.kmpgpu_alerts_read(gm._ctx, buf.ctypes.data, 0, 0) == ESTATE                       # a load drops the list
        s_rows = MM.rule_rows(s_hits, rules)
        res = check_alerts(gm, "rules", s_rows, s_counts)
        assert res["n_found"] == int(s_rows.sum()) < first["n_found"]
        # the context's counters under OPT_ACCUMULATE are untouched
        gm.set_option(OPT_ACCUMULATE, 1)
        gm.counts_reset()
        gm.scan()
        gm.scan()
        total = gm.counts_read().tolist()
        assert total == [2 * x for x in s_counts]
        check_alerts(gm, "rules", s_rows, s_counts)
        check_alerts(gm, "patterns", s_hits, s_counts)
        assert gm.counts_read().tolist() == total
        gm.set_option(OPT_ACCUMULATE, 0)
        # streaming kernels only
        for key, value in ((OPT_MODE, MODE_AUTOMATON), (OPT_KERNEL, KERNEL_GENERAL)):
            gm.set_option(key, value)
            assert scan_raw(gm, ALERT_RULES)[0] == EINVAL
            reset(gm)
        # a failed pass leaves no list; patterns drop it
        assert g.kmpgpu_alerts_read(gm._ctx, buf.ctypes.data, 0, 0) == ESTATE
        check_alerts(gm, "rules", s_rows, s_counts)
        assert g.kmpgpu_alerts_read(gm._ctx, buf.ctypes.data, 0, 1) == 0
        gm.set_patterns(TOKENS)
        assert g.kmpgpu_alerts_read(gm._ctx, buf.ctypes.data, 0, 0) == ESTATE
        # n_pkts == 0: everything 0, nothing launched, an empty list exists
        gm.load_arena(np.zeros(64, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint32))
        res = gm.scan_alerts("patterns")
        assert res["n_found"] == 0 and res["n_packets"] == 0 and res["alerts"].size == 0 and res["timing"].launches == 0
        assert not res["pkt_counts"].any() and not res["counts"].any()
        assert g.kmpgpu_alerts_read(gm._ctx, buf.ctypes.data, 0, 0) == 0
        assert g.kmpgpu_alerts_read(gm._ctx, buf.ctypes.data, 0, 1) == EINVAL
    finally:
        reset(gm)


def test_timing_and_profile(gm):
    """launches = the family's own + 4; under a profile the list kernels are the last three entries"""
    try:
        reset(gm)
        gm.set_patterns(TOKENS)
        load16(gm, random_hits(5, 500, 0.3))
        gm.set_rules(rules_of(5))
        for family, sibling in (("patterns", gm.scan_packets), ("rules", gm.scan_rules)):
            own = sibling()["timing"].launches
            gm.profile_begin(64)
            res = gm.scan_alerts(family)
            ms = gm.profile_end(64)
            assert res["n_found"] > 0 and res["timing"].launches == own + 4
            assert res["timing"].kernel_ms > 0
            assert len(ms) == own + 3 and (ms >= 0).all()     # count, the two scan kernels as one entry, fill
            assert gm.scan_alerts(family, max_records=0)["timing"].launches == own + 3
    finally:
        reset(gm)


# ------------------------------------------------------------------------------------------------
# 6. the command lines write their files from the list
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def capture_lists(tokens):
    """udp_1000.pcap x the 97 tokens and 40 generated rules: the rules, and the two lists as the Python call gives them"""
    arena = K.HostArena.from_pcap(os.path.join(DATA, "udp_1000.pcap"), "udp")
    payloads = [arena.payload(k) for k in range(arena.n_pkts)]
    hits = MM.hits(MM.starts(payloads, tokens))
    rng = random.Random(77)
    live = [i for i in range(len(tokens)) if hits[i].any()]
    rules = []
    for _ in range(40):
        pos = [rng.choice(live) for _ in range(rng.randrange(0, 3))]
        neg = [rng.choice(live) for _ in range(rng.randrange(0 if pos else 1, 3))]
        rules.append((pos, neg))
    with GpuMatcher(0) as m:
        m.set_patterns(tokens)
        m.load_arena(arena)
        m.set_rules(rules)
        pk = pairs(m.scan_alerts("patterns")["alerts"])
        al = pairs(m.scan_alerts("rules")["alerts"])
    assert pk == expected(hits) and al == expected(MM.rule_rows(hits, rules)) and pk and al
    return rules, pk, al


@pytest.mark.parametrize("prog,extra", [("serial", []), ("openmp_data", ["1"])])
def test_cli_files(capture_lists, tmp_path, prog, extra):
    rules, pk, al = capture_lists
    (tmp_path / "rules.txt").write_text("".join(" ".join([str(i) for i in pos] + [f"!{i}" for i in neg]) + "\n" for pos, neg in rules))
    packets, alerts = tmp_path / "packets.csv", tmp_path / "alerts.csv"
    r = run_cli(prog, extra=extra, env_extra={"KMPGPU_PACKETS_FILE": str(packets)})
    assert r.returncode == 0, r.stderr
    assert packets.read_text() == "".join(f"{k},{i}\n" for k, i in pk)
    r = run_cli(prog, extra=extra, env_extra={"KMPGPU_RULES_FILE": str(tmp_path / "rules.txt"), "KMPGPU_ALERTS_FILE": str(alerts)})
    assert r.returncode == 0, r.stderr
    assert alerts.read_text() == "".join(f"{k},{i}\n" for k, i in al)
