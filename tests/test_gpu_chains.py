"""Content chains (kmpgpu_set_chains, kmpgpu_scan_chains, GpuMatcher.set_chains) on a real MI355X: every content measured from the match
of the content before it.

The expectation is the host model: tests/match_model.py for the starts of every pattern, the hit matrix and the relation rows,
tests/chain_model.py for the chain rows over them.  counts come from the CPU oracle.  Every comparison is exact.

Run on a real MI355X:  python -m pytest tests/test_gpu_chains.py -m gpu
"""
import os
import random

import numpy as np
import pytest

from conftest import DATA, GOLDEN

pytestmark = pytest.mark.gpu

from gpu_support import KERNELS, attach_slots, check_relations, check_rules, gm, reset, run_cli, strip_elapsed  # noqa: E402,F401  (torch first)

import chain_model as CM  # noqa: E402
import match_model as MM  # noqa: E402
import multithreading_string_matching_amd as K  # noqa: E402
from match_model import I32_MAX, I32_MIN, U32_MAX  # noqa: E402
from multithreading_string_matching_amd import _lib  # noqa: E402
from multithreading_string_matching_amd.matcher import (  # noqa: E402
    KERNEL_AUTO, OPT_ACCUMULATE, OPT_FUSED, OPT_KERNEL, OPT_REPACK, OPT_WHOLE_PAYLOAD, GpuMatcher)

ALPHABET = b"abcdAB"
EINVAL, ESTATE = -2, -3


def check_chains(gm, rows, counts):
    res = gm.scan_chains(hits=True)
    bad = np.argwhere(res["hits"] != rows)
    assert bad.size == 0, [(int(c), int(k), bool(rows[c, k]), gm.chains[int(c)]) for c, k in bad[:8]]
    assert res["chain_pkt_counts"].tolist() == rows.sum(axis=1).tolist()
    assert res["any"].tolist() == rows.any(axis=0).tolist()
    assert res["counts"].tolist() == list(counts)
    return res


def check_kernels(gm, oracle, payloads, pats, chains, windows=None, nocase=None, whole=False, kernels=KERNELS):
    st = MM.starts(payloads, pats, windows, nocase, whole)
    hits, rows = MM.hits(st), CM.chain_rows(st, pats, chains)
    counts = MM.oracle_counts(oracle, payloads, pats, nocase, whole)
    for name, kernel, fused in kernels:
        gm.set_option(OPT_KERNEL, kernel); gm.set_option(OPT_FUSED, fused)
        check_chains(gm, rows, counts)
    gm.set_option(OPT_KERNEL, KERNEL_AUTO); gm.set_option(OPT_FUSED, 2)
    return hits, rows, counts


def candidates(hits, chains):
    """bool[n_chains, n_pkts]: the payloads that hold every content of the chain"""
    return np.array([np.logical_and.reduce([hits[p] for p, _, _ in CM.links(ch)]) for ch in chains])


def place(L, items, fill=b"abcd", rng=None):
    """a payload of L bytes of filler with the (offset, bytes) items written into it (all of them fit)"""
    b = bytearray((rng.choice(fill) if rng else fill[i % len(fill)]) for i in range(L))
    for s, p in items:
        assert 0 <= s and s + len(p) <= L, (s, len(p), L)
        b[s:s + len(p)] = p
    return bytes(b)


def three_patterns(rng, lens):
    """no letter of the filler, and the last byte of each nowhere else: a planted pattern starts where it was put and nowhere else"""
    return [bytes(rng.choice(b"EFGH") for _ in range(m - 1)) + last for m, last in zip(lens, (b"X", b"Y", b"Z"))]


def set_chains_raw(gm, chains):
    """through the C-ABI, the open sides as INT32_MIN / INT32_MAX; returns the call's return code"""
    off, flat = CM.flat_chains(chains)
    arr = (_lib.ChainLink * max(len(flat), 1))()
    for l, (p, lo, hi) in zip(arr, flat):
        l.pattern, l.dmin, l.dmax = p, lo, hi
    u32p = _lib.GPU_API["kmpgpu_set_chains"][1][1]
    return _lib.gpu_lib().kmpgpu_set_chains(gm._ctx, off.ctypes.data_as(u32p), arr, len(chains))


A3, B3, C4 = b"EFX", b"GHY", b"EGGZ"


# ------------------------------------------------------------------------------------------------
# 1. the discriminator: what no rule over relations can say
# ------------------------------------------------------------------------------------------------
def test_chain_is_not_a_rule_of_relations(gm, oracle):
    pats = [A3, B3, C4]
    chain = (0, (1, 0, 10), (2, 0, 10))
    two, one = [], []
    for s in (0, 1, 40, 57, 61, 62, 63, 64, 120, 127, 128, 700):
        for gap in (20, 64, 130, 500):
            # A .. B1 ...... B2 .. C: (A, B1) and (B2, C) in range, B1 too far in front of C, B2 too far behind A
            two.append(place(s + gap + 40, [(s, A3), (s + 5, B3), (s + 5 + gap, B3), (s + 5 + gap + 6, C4)]))
        one.append(place(s + 40, [(s, A3), (s + 5, B3), (s + 11, C4)]))      # one B serves both
        one.append(place(s + 300, [(s, A3), (s + 5, B3), (s + 11, C4), (s + 200, B3)]))
    payloads = two + one + [place(100, [(5, A3), (12, B3)]), place(100, [(5, B3), (12, C4)]), b""]
    relations = CM.pairwise_relations(chain)
    st = MM.starts(payloads, pats)
    hits, rel_rows, rows = MM.hits(st), MM.relation_rows(st, pats, relations), CM.chain_rows(st, pats, [chain])
    n2, n1 = len(two), len(one)
    assert rel_rows[:, :n2 + n1].all()                                     # both relations hold in both kinds of payload
    assert not rows[0, :n2].any() and rows[0, n2:n2 + n1].all() and not rows[0, n2 + n1:].any()
    try:
        reset(gm)
        gm.set_patterns(pats)
        gm.load_arena(K.HostArena.from_payloads(payloads))
        gm.set_relations(relations)
        gm.set_chains([chain])
        assert gm.chains == [chain]
        rules = [([gm.rel(0), gm.rel(1)], []), ([gm.chain(0)], []), ([gm.rel(0), gm.rel(1)], [gm.chain(0)])]
        gm.set_rules(rules)
        counts = MM.oracle_counts(oracle, payloads, pats)
        mat = np.concatenate([hits, rel_rows, rows])
        for _, kernel, fused in KERNELS:
            gm.set_option(OPT_KERNEL, kernel); gm.set_option(OPT_FUSED, fused)
            check_chains(gm, rows, counts)
            got = check_rules(gm, mat, rules, counts)["hits"]
            # the rule over the relations fires on both kinds, the chain on one; the third rule is exactly the false alerts
            assert got[0, :n2 + n1].all() and not got[1, :n2].any() and got[1, n2:n2 + n1].all()
            assert got[2, :n2].all() and not got[2, n2:].any()
    finally:
        reset(gm)


# ------------------------------------------------------------------------------------------------
# 2. link bound edges: d = dmin - 1, dmin, dmax, dmax + 1 on one link, the other one satisfied
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", [(1, 1, 1), (99, 99, 99), (3, 17, 4)])
def test_link_bound_edges(gm, oracle, lens):
    rng = random.Random(f"edges-{lens}")
    pats = three_patterns(rng, lens)
    ranges = [(0, 0), (0, 20), (5, 5), (1, 70), (None, 7), (3, None), (None, None), (63, 64), (64, None), (200, 1000)]
    ok = (2, 9)                                       # the range of the link that is not under test; its d is 5
    chains = [(0, (1, lo, hi), (2, *ok)) for lo, hi in ranges] + [(0, (1, *ok), (2, lo, hi)) for lo, hi in ranges]
    payloads = []
    sa = 70
    for lo, hi in ranges:
        for d in sorted({x for x in (None if lo is None else lo - 1, lo, hi, None if hi is None else hi + 1) if x is not None and x >= 0}):
            for d1, d2 in ((d, 5), (5, d)):
                sb = sa + lens[0] + d1
                sc = sb + lens[1] + d2
                payloads.append(place(sc + lens[2] + rng.randrange(0, 40), [(sa, pats[0]), (sb, pats[1]), (sc, pats[2])], rng=rng))
    payloads += [place(700, [(sa, pats[0]), (300, pats[1])]), place(700, [(sa, pats[2])]), b""]
    try:
        reset(gm)
        gm.set_patterns(pats)
        gm.load_arena(K.HostArena.from_payloads(payloads))
        gm.set_chains(chains)
        assert gm.chains == chains
        hits, rows, _ = check_kernels(gm, oracle, payloads, pats, chains)
        cand = candidates(hits, chains)
        assert rows.any(axis=1).all()                 # every chain holds somewhere and fails on a payload that holds all three contents
        assert (cand & ~rows).any(axis=1).all()
        # the raw INT32 ends through the C-ABI are the same open sides
        raw = [c for c in chains if None in c[1] or None in c[2]]
        assert len(raw) == 8 and set_chains_raw(gm, raw) == 0
        gm.chains = raw
        res = gm.scan_chains(hits=True)
        assert (res["hits"] == rows[[chains.index(c) for c in raw]]).all()
    finally:
        reset(gm)


# ------------------------------------------------------------------------------------------------
# 3. step edges of the sweep
# ------------------------------------------------------------------------------------------------
def test_sweep_step_edges(gm, oracle):
    rng = random.Random("steps")
    D, F = b"PQRS", b"RSTU"                            # PQRSTU holds D at 0 and F at 2: d = -2
    pats = [A3, B3, C4, D, F]
    gaps = [(0, 0), (1, 0), (0, 1), (64, 0), (0, 64), (61, 61), (57, 60)]
    payloads = []
    # consecutive matches straddle the 64-offset steps
    for s in (0, 1, 62, 63, 64, 65, 127, 128):
        for g1, g2 in gaps:
            sb = s + 3 + g1
            sc = sb + 3 + g2
            payloads.append(place(sc + 4 + rng.randrange(0, 70), [(s, A3), (sb, B3), (sc, C4)], rng=rng))
        # a link that reaches backwards: B in front of A, C behind A
        payloads.append(place(s + 90, [(s, B3), (s + 7, A3), (s + 20, C4)], rng=rng))
        payloads.append(place(s + 90, [(s + 66, B3), (s, A3), (s + 80, C4)], rng=rng))
        # overlapping contents
        payloads.append(place(s + 40, [(s, b"PQRSTU"), (s + 9, A3)], rng=rng))
        payloads.append(place(s + 40, [(s, b"PQRSTU"), (s + 30, A3)], rng=rng))
        payloads.append(place(s + 40, [(s, D), (s + 10, F), (s + 20, A3)], rng=rng))
    # the payload's length: A at its start, C at its end
    total = 3 + 3 + 4
    for L in (0, 1, total - 1, total, 63, 64, 65, 129, 2200):
        if L < total:
            payloads.append(place(L, [(0, A3)] if L >= 3 else []))
            continue
        payloads.append(place(L, [(0, A3), (L // 2 - 1, B3), (L - 4, C4)], rng=rng))
        payloads.append(place(L, [(L - 3, A3), (L // 2 - 1, B3), (0, C4)], rng=rng))          # and the other way round
    chains = [(0, (1, g1, g1), (2, g2, g2)) for g1, g2 in gaps]
    chains += [(0, (1, 0, 1), (2, 0, 1)), (0, (1, None, 0), (2, 0, None)), (0, (1, 0, None), (2, 0, None)), (0, (1, None, None), (2, None, None)),
               (0, (1, 2, 63), (2, 2, 63)), (0, (1, 64, None), (2, None, 0)),
               (0, (1, -10, -10), (2, 17, 17)), (0, (1, -20, -8), (2, 0, 30)), (0, (1, 63, 63), (2, 11, 11)), (0, (1, None, -1), (2, None, None)),
               (2, (1, None, -1), (0, None, -1)), (2, (1, None, None), (0, None, None)),
               (3, (4, -2, -2), (0, 3, 3)), (3, (4, -2, -2), (0, 4, None)), (3, (4, 6, 6), (0, 6, 6)), (4, (3, -6, -6), (0, 5, 5)), (3, (4, -1, 6), (0, 5, 6))]
    try:
        reset(gm)
        gm.set_patterns(pats)
        gm.load_arena(K.HostArena.from_payloads(payloads))
        gm.set_chains(chains)
        hits, rows, _ = check_kernels(gm, oracle, payloads, pats, chains)
        assert rows.any(axis=1).all()
        assert (candidates(hits, chains) & ~rows).any(axis=1).sum() >= len(chains) - 2        # (the two fully open ones hold in every candidate)
    finally:
        reset(gm)


# ------------------------------------------------------------------------------------------------
# 4. length edges: 2, 3, 7 and 8 contents at once
# ------------------------------------------------------------------------------------------------
def _length_case():
    rng = random.Random("lengths-1")
    pats = [b"a", b"b", b"ab", b"c", b"ca", b"d", b"bd", b"dd"]
    payloads = [bytes(rng.choice(b"abcd") for _ in range(rng.choice([0, 9, 30, 70, 200]))) for _ in range(150)]
    chains = []
    for n in (2, 3, 7, 8, 8, 7, 3, 2):
        ch = [rng.randrange(8)]
        for _ in range(n - 1):
            lo = rng.randrange(-6, 6)
            ch.append((rng.randrange(8), lo, lo + rng.randrange(2, 9)))
        chains.append(tuple(ch))
    return pats, payloads, chains


def test_length_edges(gm, oracle):
    pats, payloads, chains = _length_case()
    try:
        reset(gm)
        gm.set_patterns(pats)
        gm.load_arena(K.HostArena.from_payloads(payloads))
        gm.set_chains(chains)
        hits, rows, counts = check_kernels(gm, oracle, payloads, pats, chains)
        assert rows.any(axis=1).all() and (candidates(hits, chains) & ~rows).any(axis=1).all()
        # a chain of two contents is the relation, bit for bit
        two = [c for c, ch in enumerate(chains) if len(ch) == 2]
        gm.set_relations([CM.pairwise_relations(chains[c])[0] for c in two])
        rel = gm.scan_relations(hits=True)
        got = gm.scan_chains(hits=True)
        assert np.array_equal(rel["hits"], got["hits"][two]) and rel["rel_pkt_counts"].tolist() == got["chain_pkt_counts"][two].tolist()
        assert gm.chains == chains                    # set_relations keeps the chains
        # nine contents and one content
        for bad in ([tuple([0] + [(1, 0, 5)] * 8)], [(0,)], [chains[0], (3,)], [chains[0], tuple([0] + [(1, None, None)] * 8)]):
            assert set_chains_raw(gm, bad) == EINVAL, bad
            assert b"kmpgpu_set_chains" in _lib.gpu_lib().kmpgpu_last_error()
        check_chains(gm, rows, counts)
        assert set_chains_raw(gm, [tuple([0] + [(1, 0, 5)] * 7)]) == 0
    finally:
        reset(gm)


# ------------------------------------------------------------------------------------------------
# 5. one pattern several times in a chain
# ------------------------------------------------------------------------------------------------
def test_repeats(gm, oracle):
    pats = [A3, B3]
    payloads = [
        place(120, [(10, A3), (18, A3), (26, A3)]),          # three occurrences, d = 5 and 5
        place(120, [(10, A3), (18, A3)]),                    # two
        place(120, [(10, A3)]),                              # one: pairs with itself where -3 is in range
        place(300, [(10, A3), (30, A3), (38, A3)]),          # behind 38 the nearest earlier match (30, d = 5) is out of range, 10 (d = 25) is in
        place(300, [(10, A3), (30, A3), (38, A3), (45, B3)]),
        place(200, [(s, A3) for s in range(0, 190, 3)]),     # back to back
        place(200, [(60, A3), (64, A3), (125, A3), (130, A3)]),
        b"",
    ]
    chains = [(0, (0, 5, 5), (0, 5, 5)), (0, (0, -3, -3), (0, -3, -3)), (0, (0, -3, -3), (0, 5, 5)), (0, (0, 0, None), (0, 0, None)),
              (0, (0, 20, 30)), (0, (0, 20, 30), (0, -3, -3)), (0, (0, 20, 30), (1, 0, 10)), (0, (0, 17, 17), (0, 20, 30)), (0, (0, 0, 0), (0, 0, 0), (0, 0, 0)),
              (0, (0, None, -4), (0, None, -4)), (0, (0, 1, 1), (0, 58, 58), (0, 2, 2)), (0, (0, 1, 1), (0, 58, 58), (0, 3, 3)),
              (0, (0, -3, -3), (0, -3, -3), (0, -3, -3), (0, -3, -3), (0, -3, -3), (0, -3, -3), (0, -3, -3))]
    try:
        reset(gm)
        gm.set_patterns(pats)
        gm.load_arena(K.HostArena.from_payloads(payloads))
        gm.set_chains(chains)
        _, rows, _ = check_kernels(gm, oracle, payloads, pats, chains)
        assert rows[0, :3].tolist() == [True, False, False] and rows[1, :3].all() and rows[2, :3].tolist() == [True, True, False]
        assert rows[3, :3].tolist() == [True, False, False]
        assert rows[4, 3] and rows[5, 3] and not rows[6, 3] and rows[6, 4] and not rows[7, 3]
        assert rows[8, 5] and not rows[8, 0] and rows[10, 6] and not rows[11, 6] and rows[12, 2]
    finally:
        reset(gm)


# ------------------------------------------------------------------------------------------------
# 6. a long payload: the carries run over a thousand steps
# ------------------------------------------------------------------------------------------------
def test_long_payload(gm, oracle):
    pats = [A3, B3, C4]
    L, sa, sb, sc = 66_000, 5, 33_001, 65_990
    d1, d2 = sb - (sa + 3), sc - (sb + 3)
    payloads = [place(L, [(sa, A3), (sb, B3), (sc, C4)]), place(300, [(sa, A3), (100, B3), (200, C4)]), b"",
                place(L, [(sa, A3), (sb, B3), (sc - 1, C4)]), place(L, [(sa, A3), (sb + 1, B3), (sc, C4)])]
    chains = [(0, (1, d1, d1), (2, d2, d2)), (0, (1, 0, d1), (2, 0, d2)), (0, (1, d1, None), (2, d2, None)), (0, (1, None, None), (2, None, None)),
              (0, (1, 0, d1 - 1), (2, None, None)), (0, (1, d1, d1), (2, d2 + 1, None)), (0, (1, d1 + 1, None), (2, None, d2 - 1)),
              (0, (1, 0, d1), (2, 0, d2 - 1)), (2, (1, -d2 - 7, -d2 - 7), (0, -d1 - 6, -d1 - 6)), (2, (1, None, 0), (0, -d1 - 5, 0)),
              (0, (1, 32_768, 32_993), (2, 32_768, 65_535))]
    try:
        reset(gm)
        gm.set_patterns(pats)
        gm.load_arena(K.HostArena.from_payloads(payloads))
        gm.set_chains(chains)
        _, rows, _ = check_kernels(gm, oracle, payloads, pats, chains)
        assert rows[:4, 0].all() and not rows[4:8, 0].any() and rows[8, 0] and not rows[9, 0] and rows[10, 0]
        assert rows[7, 3] and not rows[0, 3] and rows[6, 4] and not rows[0, 4]
    finally:
        reset(gm)


# ------------------------------------------------------------------------------------------------
# 7. the text's end
# ------------------------------------------------------------------------------------------------
def test_text_end(gm, oracle):
    rng = random.Random("end")
    pats = [A3, B3, C4]
    payloads = []
    for k in range(84):
        L = rng.randrange(60, 1300)
        sa = rng.randrange(0, L - 50)
        sb = rng.randrange(sa + 3, L - 20)
        sc = rng.randrange(sb + 3, L - 4)
        b = bytearray(place(L, [(sa, A3), (sb, B3), (sc, C4)], rng=rng))
        z = [None, rng.randrange(0, sa + 1), sa + 1, rng.randrange(sa + 3, sb + 1), sb + 2, rng.randrange(sb + 3, sc + 1), sc + 3, sc + 4 if sc + 4 < L else None][k % 8]
        if z is not None:
            b[z] = 0                                  # in front of A; inside A; between A and B; inside B; between B and C; inside C; directly behind C
        payloads.append(bytes(b))
    # a C that ends exactly at the payload's end, and one whose last byte lies in the slot's padding
    payloads += [place(50, [(4, A3), (20, B3), (46, C4)]), place(49, [(4, A3), (20, B3)])[:46] + C4[:3],
                 place(64, [(4, A3), (20, B3), (60, C4)]), place(63, [(4, A3), (20, B3)])[:60] + C4[:3]]
    slots = []
    for t in payloads:
        pad = (-len(t)) % 16 or (16 if not t else 0)
        slots.append(t + (b"Z" + C4 + A3 + b"Z" * 16)[:pad])          # the padding would complete the cut C
    chains = [(0, (1, 0, None), (2, 0, None)), (0, (1, None, None), (2, None, None)), (2, (1, None, None), (0, None, None)), (0, (1, 0, 400), (2, 0, 400)),
              (0, (1, 13, 13), (2, 23, 23)), (0, (1, 13, 13), (2, 37, 37))]
    try:
        reset(gm)
        gm.set_patterns(pats)
        for attach in (False, True):
            keep = attach_slots(gm, payloads, slots) if attach else gm.load_arena(K.HostArena.from_payloads(payloads))
            gm.set_chains(chains)
            seen = {}
            for whole in (0, 1, 0):                   # switched between two calls with nothing reloaded
                gm.set_option(OPT_WHOLE_PAYLOAD, whole)
                seen[whole] = check_kernels(gm, oracle, payloads, pats, chains, whole=bool(whole))[1]
            assert (seen[1] | seen[0] == seen[1]).all() and seen[1].sum() > seen[0].sum() > 0
            n = len(payloads)
            assert seen[0][4, n - 4] and not seen[0][0, n - 3] and seen[0][5, n - 2] and not seen[1][0, n - 1]
            del keep
    finally:
        reset(gm)


# ------------------------------------------------------------------------------------------------
# 8. nocase: contents read alternately from the arena and from its folded copy
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nocase", [(False, True, False), (True, False, True), (True, True, True)], ids=["b", "ac", "all"])
def test_nocase(gm, oracle, nocase):
    rng = random.Random(f"nocase-{nocase}")
    A, B, Cc = b"aBcA", b"bAd", b"Cb"
    payloads = []
    for _ in range(200):
        L = rng.randrange(0, 500)
        b = bytearray(rng.choice(b"abcdABCD") for _ in range(L))
        for _ in range(L // 50):
            p = rng.choice([A, B, Cc, A.lower(), B.upper(), A.swapcase(), Cc.swapcase()])
            s = rng.randrange(0, L - len(p) + 1)
            b[s:s + len(p)] = p
        payloads.append(bytes(b))
    pats = [A, B, Cc, b"-+-"]                          # (the fourth: a nocase pattern without a letter stays with the arena)
    flags = list(nocase) + [True]
    chains = [(0, (1, 0, 30), (2, 0, 30)), (1, (0, 0, 30), (1, 0, 30), (0, 0, 30)), (0, (1, -20, -1), (2, -20, 20)), (0, (1, None, None), (2, None, None)),
              (2, (2, 1, 100), (0, 0, 9), (1, 0, 60)), (1, (1, -3, -3), (0, 0, None)), (0, (1, 100, None), (2, None, 0)), (3, (0, None, None))]
    try:
        reset(gm)
        gm.set_patterns(pats, nocase=flags)
        gm.load_arena(K.HostArena.from_payloads(payloads))
        gm.set_chains(chains)
        hits, rows, _ = check_kernels(gm, oracle, payloads, pats, chains, nocase=flags)
        sens = CM.chain_rows(MM.starts(payloads, pats), pats, chains)
        assert rows[:7].any(axis=1).all() and (rows != sens).any()      # folding found tuples that the bytes as written do not hold
    finally:
        reset(gm)


# ------------------------------------------------------------------------------------------------
# 9. windows decide what a match is, and are pass state
# ------------------------------------------------------------------------------------------------
def test_windows(gm, oracle):
    pats = [A3, B3, C4]
    payloads = [place(400, [(10, A3), (20, B3), (30, C4), (100, B3)]),       # B at 20 serves both links, B at 100 none
                place(400, [(10, A3), (20, B3), (300, B3), (310, C4)]),      # no B serves both
                place(400, [(10, A3), (20, B3), (30, C4), (200, A3), (210, B3), (220, C4)]),
                place(90, [(10, A3), (20, B3), (30, C4)])]
    chains = [(0, (1, 0, 10), (2, 0, 10)), (0, (1, 0, None), (2, 0, 10)), (0, (1, None, None), (2, None, None)), (2, (1, None, -1), (0, None, -1))]
    try:
        reset(gm)
        gm.set_patterns(pats)
        gm.load_arena(K.HostArena.from_payloads(payloads))
        gm.set_chains(chains)
        gm.set_rules([([0, 1, gm.chain(0)], []), ([0], [gm.chain(1)])])
        base = check_kernels(gm, oracle, payloads, pats, chains)[1]
        assert base[0].tolist() == [True, False, True, True]
        for windows in ([(0, None), (50, None), (0, None)],           # removes the only B that serves both links in payloads 0 and 3
                        [(0, None), (0, None), (0, 29)], [(11, None), (0, None), (0, None)], [(0, None), (20, 20), (30, 30)], [(0, 10), (0, 20), (220, 220)]):
            gm.set_windows(windows)
            hits, rows, counts = check_kernels(gm, oracle, payloads, pats, chains, windows=windows)
            assert (rows != base).any()
            check_rules(gm, np.concatenate([hits, rows]), gm.rules, counts)            # the rules, set before the windows, stay valid
            gm.set_windows(None)                                     # cleared between two passes, nothing re-set
            assert (check_kernels(gm, oracle, payloads, pats, chains)[1] == base).all()
        gm.set_windows([(0, None), (50, None), (0, None)])
        got = gm.scan_chains(hits=True)["hits"]
        assert not got[0, 0] and not got[0, 3] and got[0, 2]
    finally:
        reset(gm)


# ------------------------------------------------------------------------------------------------
# 10. column and row edges
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_pkts", [1, 63, 64, 65, 129])
def test_column_edges(gm, oracle, n_pkts):
    pats = [A3, B3, C4]
    payloads = []
    for k in range(n_pkts):
        r = k % 7 if k < n_pkts - 1 else 0              # candidates in the last payload
        d = [4, 30, 4, 4, 30, 4, 4][r]
        payloads.append(place(40 + d + (k % 50), [(2, A3), (5 + d, B3), (12 + d, C4)]) if r in (0, 1, 4) else place(10 + k % 30, [(2, A3)] if r == 2 else []))
    chains = [(0, (1, 0, 10), (2, 4, 4)), (0, (1, 11, 40), (2, 0, 9)), (2, (1, None, None), (0, None, None)), (0, (1, 5, 29), (2, 4, 4))]
    try:
        reset(gm)
        gm.set_patterns(pats)
        gm.load_arena(K.HostArena.from_payloads(payloads))
        gm.set_chains(chains)
        hits, rows, counts = check_kernels(gm, oracle, payloads, pats, chains)
        assert rows[0, n_pkts - 1] and not rows[3].any()
        # the words as the C-ABI writes them: bits at n_pkts and above are 0
        W = (n_pkts + 63) // 64
        rc, any_w, hit_w = np.full(4, 7, np.uint64), np.full(W, U32_MAX, np.uint64), np.full((4, W), U32_MAX, np.uint64)
        assert _lib.gpu_lib().kmpgpu_scan_chains(gm._ctx, rc.ctypes.data, any_w.ctypes.data, hit_w.ctypes.data, None, None) == 0
        bits = np.unpackbits(hit_w.view(np.uint8), axis=1, bitorder="little")
        assert (bits[:, :n_pkts].astype(bool) == rows).all() and not bits[:, n_pkts:].any()
        abits = np.unpackbits(any_w.view(np.uint8), bitorder="little")
        assert (abits[:n_pkts].astype(bool) == rows.any(axis=0)).all() and not abits[n_pkts:].any()
        assert rc.tolist() == rows.sum(axis=1).tolist()
    finally:
        reset(gm)


@pytest.mark.parametrize("n_chains", [1, 257])
def test_row_edges(gm, oracle, n_chains):
    rng = random.Random(f"rows-{n_chains}")
    pats = [A3, B3, b"ab", b"c"]
    payloads = []
    for k in range(100):
        L = rng.randrange(0, 120)
        b = bytearray(rng.choice(b"abcd") for _ in range(L))
        for p in pats[:2]:
            if L >= 10 and rng.random() < 0.7:
                s = rng.randrange(0, L - 3)
                b[s:s + 3] = p
        payloads.append(bytes(b))
    kinds = [(0, (1, 0, 20), (2, 0, 9)), (0, (1, 0, 20), (2, 0, 9)), (1, (0, 0, 20)), (2, (3, 0, 0), (2, 0, 0)), (3, (2, -1, 4), (3, 0, 3), (2, 0, 3)), (2, (2, 2, 9)),
             (0, (2, None, -3), (1, None, None)), (3, (1, 5, None), (3, None, 9))]
    chains = []
    for q in range(n_chains):
        if q % 3:
            chains.append(kinds[q % len(kinds)])
        else:
            chains.append(tuple([rng.randrange(4)] + [(rng.randrange(4), -rng.randrange(0, 9), rng.randrange(0, 30)) for _ in range(rng.randrange(1, 4))]))
    try:
        reset(gm)
        gm.set_patterns(pats)
        gm.load_arena(K.HostArena.from_payloads(payloads))
        gm.set_chains(chains)
        _, rows, _ = check_kernels(gm, oracle, payloads, pats, chains, kernels=KERNELS[:1])
        assert rows.any() and not rows.all()
    finally:
        reset(gm)


# ------------------------------------------------------------------------------------------------
# 11. random differential
# ------------------------------------------------------------------------------------------------
def _random_case(seed, n_chains=30):
    rng = random.Random(f"diff-{seed}")
    pats = [bytes(rng.choice(ALPHABET) for _ in range(m)) for m in (1, 2, 2, 3, 4, 5)]
    chains = []
    for _ in range(n_chains):
        ch = [rng.randrange(6)]
        for _ in range(rng.randrange(1, 5)):
            lo = rng.randrange(-40, 40)
            ch.append((rng.randrange(6), None if rng.random() < 0.1 else lo, None if rng.random() < 0.1 else lo + rng.randrange(0, 30)))
        chains.append(tuple(ch))
    return rng, pats, chains


def _random_payloads(rng, kind, n=300):
    payloads = []
    for _ in range(n):
        L = 333 if kind == "uniform" else 0 if (kind == "empty" and rng.random() < 0.5) else rng.randrange(0, 401)
        b = bytearray(rng.choice(ALPHABET) for _ in range(L))
        if L and rng.random() < 0.3:
            b[rng.randrange(L)] = 0
        payloads.append(bytes(b))
    return payloads


def fails_though_every_link_holds(st, pats, chains, rows):
    """(chain, payload) pairs in which every pairwise relation of the chain holds and the chain does not"""
    n = 0
    for c, ch in enumerate(chains):
        n += int((MM.relation_rows(st, pats, CM.pairwise_relations(ch)).all(axis=0) & ~rows[c]).sum())
    return n


@pytest.mark.parametrize("kind", ["uniform", "mixed", "empty", "dirty", "in_place"])
@pytest.mark.parametrize("seed", [1, 2])
def test_random_differential(gm, oracle, seed, kind):
    rng, pats, chains = _random_case(seed)
    payloads = _random_payloads(rng, kind)
    keep = None
    try:
        reset(gm)
        gm.set_patterns(pats)
        if kind == "dirty":
            slots = [t + bytes(rng.choice(ALPHABET) for _ in range((-len(t)) % 16 or (16 if not t else 0))) for t in payloads]
            keep = attach_slots(gm, payloads, slots)
        elif kind == "in_place":
            # OPT_REPACK = 0: slots with gaps, not in payload order; the marking pass packs such an arena on the call
            ln = np.array([len(t) for t in payloads], dtype=np.uint32)
            slot = np.maximum(16, (ln.astype(np.uint64) + 15) // 16 * 16) + 32
            order = list(range(len(payloads)))
            rng.shuffle(order)
            off, pos = np.zeros(len(payloads), dtype=np.uint64), 0
            for k in order:
                off[k] = pos
                pos += int(slot[k])
            arena = np.frombuffer(bytes(rng.choice(ALPHABET) for _ in range(pos)) + b"\0" * 64, dtype=np.uint8).copy()
            for k, t in enumerate(payloads):
                arena[int(off[k]):int(off[k]) + len(t)] = np.frombuffer(t, dtype=np.uint8)
            gm.set_option(OPT_REPACK, 0)
            gm.load_arena(arena, off, ln)
        else:
            gm.load_arena(K.HostArena.from_payloads(payloads))
        gm.set_chains(chains)
        for whole in (0, 1):
            gm.set_option(OPT_WHOLE_PAYLOAD, whole)
            hits, rows, _ = check_kernels(gm, oracle, payloads, pats, chains, whole=bool(whole))
            assert rows.any() and (candidates(hits, chains) & ~rows).any()
            # what no rule over relations tells apart: every link holds on its own, the chain does not
            assert fails_though_every_link_holds(MM.starts(payloads, pats, whole=bool(whole)), pats, chains, rows) > 0
    finally:
        reset(gm)
        del keep


# ------------------------------------------------------------------------------------------------
# 12. rules over chains
# ------------------------------------------------------------------------------------------------
def test_rules_over_chains(gm, oracle):
    rng, pats, chains = _random_case(7)
    payloads = _random_payloads(rng, "empty")
    relations = [(0, 1, 0, 30), (2, 3, None, 5), (4, 4, 1, None)]
    windows = [(0, None), (3, 200), (0, None), (0, 100), (0, None), (1, None)]
    try:
        reset(gm)
        gm.set_patterns(pats)
        gm.load_arena(K.HostArena.from_payloads(payloads))
        gm.set_relations(relations)
        pattern_rules = [([0, 3], [4]), ([], [5]), ([gm.rel(0)], [gm.rel(2)])]
        gm.set_rules(pattern_rules)
        before = (gm.scan_packets(hits=True), gm.scan_rules(hits=True), gm.scan_relations(hits=True))
        gm.set_chains(chains)
        assert gm.rules == [] and gm.relations == relations
        Ch, R = gm.chain, gm.rel
        assert Ch(0) == len(pats) + len(relations)
        # a chain that holds in some of the payloads that hold all of its contents: as a term it narrows the AND of its contents
        st0 = MM.starts(payloads, pats)
        hits0, rows0 = MM.hits(st0), CM.chain_rows(st0, pats, chains)
        cand0 = candidates(hits0, chains)
        qn = next(c for c in range(len(chains)) if rows0[c].any() and (cand0[c] & ~rows0[c]).any())
        contents = sorted({p for p, _, _ in CM.links(chains[qn])})
        rules = [(contents + [Ch(qn)], []), (contents, [Ch(qn)]), ([], [Ch(1)]), ([Ch(2), Ch(3)], []), ([Ch(4), R(0)], [Ch(5), 0]),
                 ([Ch(6), Ch(7), Ch(8), Ch(9), 1, 2], [Ch(10), R(1)]), ([Ch(29)], []), ([], [Ch(11), Ch(12), R(2)])]
        gm.set_rules(rules)
        for w in (None, windows):
            gm.set_windows(w)
            hits, rows, counts = check_kernels(gm, oracle, payloads, pats, chains, windows=w)
            rel_rows = MM.relation_rows(MM.starts(payloads, pats, w), pats, relations)
            mat = np.concatenate([hits, rel_rows, rows])
            for _, kernel, fused in KERNELS:
                gm.set_option(OPT_KERNEL, kernel); gm.set_option(OPT_FUSED, fused)
                check_rules(gm, mat, rules, counts)
                check_relations(gm, rel_rows, counts)
            gm.set_option(OPT_KERNEL, KERNEL_AUTO); gm.set_option(OPT_FUSED, 2)      # (as `before` was taken: the launches are compared below)
            want = MM.rule_rows(mat, rules)
            empty = np.array([len(t) == 0 for t in payloads])
            assert want[2][empty].all() and empty.any()                 # all-negated: empty payloads match
            if w is None:
                assert want[0].any() and want[1].any()
        gm.set_windows(None)
        # the pattern-level and relation-level calls return what they returned before there were chains
        gm.scan_chains()
        pk, rl = gm.scan_packets(hits=True), gm.scan_relations(hits=True)
        gm.set_rules(pattern_rules)
        ru = gm.scan_rules(hits=True)
        for got, was in ((pk, before[0]), (ru, before[1]), (rl, before[2])):
            for key in was:
                if key != "timing":
                    assert np.array_equal(got[key], was[key]), key
        assert ru["timing"].launches == before[1]["timing"].launches + 1            # the chain kernel runs while chains are set
        gm.set_chains(None)
        assert gm.chains == [] and gm.rules == [] and gm.relations == relations
        gm.set_rules(pattern_rules)
        ru = gm.scan_rules(hits=True)
        assert all(np.array_equal(ru[key], before[1][key]) for key in before[1] if key != "timing")
        assert ru["timing"].launches == before[1]["timing"].launches
    finally:
        reset(gm)


# ------------------------------------------------------------------------------------------------
# 13. state and errors
# ------------------------------------------------------------------------------------------------
def test_state_and_errors(gm, oracle):
    rng, pats, chains = _random_case(11, n_chains=5)
    payloads = _random_payloads(rng, "mixed", n=150)
    relations = [(0, 1, 0, 30), (2, 3, None, 5)]
    g = _lib.gpu_lib()
    u32p = _lib.GPU_API["kmpgpu_set_rules"][1][1]

    def raw(ctx, off, flat, n):
        arr = (_lib.ChainLink * max(len(flat), 1))()
        for l, (p, lo, hi) in zip(arr, flat):
            l.pattern, l.dmin, l.dmax = p, lo, hi
        off = np.array(off, dtype=np.uint32)
        return g.kmpgpu_set_chains(ctx, off.ctypes.data_as(u32p), arr, n)

    OPEN = (I32_MIN, I32_MAX)
    try:
        reset(gm)
        with GpuMatcher(0) as fresh:
            assert raw(fresh._ctx, [0, 2], [(0, *OPEN), (0, 0, 0)], 1) == ESTATE          # no patterns set
            assert g.kmpgpu_set_chains(fresh._ctx, None, None, 0) == ESTATE
            assert g.kmpgpu_scan_chains(fresh._ctx, None, None, None, None, None) == ESTATE
            fresh.set_patterns(pats)
            fresh.load_arena(K.HostArena.from_payloads(payloads))
            assert g.kmpgpu_scan_chains(fresh._ctx, None, None, None, None, None) == ESTATE      # no chains set
            assert b"kmpgpu_scan_chains" in g.kmpgpu_last_error()
            with pytest.raises(Exception):
                fresh.chain(0)
        n = len(pats)
        gm.set_patterns(pats)
        gm.load_arena(K.HostArena.from_payloads(payloads))
        gm.set_relations(relations)
        gm.set_chains(chains)
        nt = n + len(relations) + len(chains)              # rows a term can name
        rules = [([0, gm.chain(0)], []), ([gm.rel(1)], [gm.chain(4)])]
        gm.set_rules(rules)
        st = MM.starts(payloads, pats)
        hits, rel_rows, rows = MM.hits(st), MM.relation_rows(st, pats, relations), CM.chain_rows(st, pats, chains)
        mat = np.concatenate([hits, rel_rows, rows])
        counts = MM.oracle_counts(oracle, payloads, pats)

        def in_force():
            check_chains(gm, rows, counts)
            check_rules(gm, mat, rules, counts)

        # every refused call leaves the chains and the rules set before in force
        good = [(0, *OPEN), (1, 0, 5)]
        for off, flat in (([1, 3], [(0, *OPEN)] + good),                                   # chain_off[0] != 0
                          ([0, 2, 1], good), ([0, 4, 2], good + good),                     # a decreasing chain_off
                          ([0, 1], good), ([0, 2, 2], good), ([0, 0], good),               # fewer than 2 links
                          ([0, 9], [(0, *OPEN)] + [(1, 0, 5)] * 8),                        # more than 8
                          ([0, 2], [(n, *OPEN), (1, 0, 5)]), ([0, 2], [(0, *OPEN), (n, 0, 5)]), ([0, 2, 4], good + [(0, *OPEN), (U32_MAX, 0, 5)]),
                          ([0, 2], [(0, *OPEN), (1, 5, 4)]), ([0, 3], good + [(1, I32_MAX, I32_MIN)]),           # dmin > dmax
                          ([0, 2], [(0, 0, I32_MAX), (1, 0, 5)]), ([0, 2], [(0, I32_MIN, 7), (1, 0, 5)]), ([0, 2, 4], good + [(0, 0, 0), (1, 0, 5)])):   # bounds on a first link
            assert raw(gm._ctx, off, flat, len(off) - 1) == EINVAL, (off, flat)
            assert b"kmpgpu_set_chains" in g.kmpgpu_last_error()
            in_force()
        off2 = np.array([0, 2], dtype=np.uint32)
        one = (_lib.ChainLink * 2)()
        one[0].pattern, one[0].dmin, one[0].dmax = 0, I32_MIN, I32_MAX
        one[1].pattern, one[1].dmin, one[1].dmax = 1, 0, 5
        assert g.kmpgpu_set_chains(gm._ctx, None, one, 1) == EINVAL and g.kmpgpu_set_chains(gm._ctx, off2.ctypes.data_as(u32p), None, 1) == EINVAL
        # too many rows: n_pat + n_rel + n_chains has to stay below 2^31 (checked before the arrays are read)
        for n_ch in ((1 << 31) - n - len(relations), (1 << 32) - n - len(relations), U32_MAX):
            assert g.kmpgpu_set_chains(gm._ctx, off2.ctypes.data_as(u32p), one, n_ch) == EINVAL, n_ch
            assert b"kmpgpu_set_chains" in g.kmpgpu_last_error()
        in_force()
        with pytest.raises(Exception):
            gm.set_chains([(0, (n, 0, 0))])
        assert gm.chains == chains and gm.rules == rules
        in_force()
        # the bound of a rule's term is n_pat + n_rel + n_chains
        off = np.array([0, 1], dtype=np.uint32)
        for term, rc in ((nt, EINVAL), (nt | _lib.RULE_NOT, EINVAL), (nt - 1, 0)):
            t = np.array([term], dtype=np.uint32)
            assert g.kmpgpu_set_rules(gm._ctx, off.ctypes.data_as(u32p), t.ctypes.data_as(u32p), 1) == rc, term
        gm.rules = [([nt - 1], [])]
        check_rules(gm, mat, gm.rules, counts)
        # a successful kmpgpu_set_chains drops the rules: the same chains again, and a clear
        for chs in (chains, []):
            gm.set_rules(rules if chs else [([0], [])])
            gm.set_chains(chs)
            assert gm.rules == [] and gm.relations == relations
            assert g.kmpgpu_scan_rules(gm._ctx, None, None, None, None, None) == ESTATE
        assert g.kmpgpu_scan_chains(gm._ctx, None, None, None, None, None) == ESTATE
        t = np.array([n + len(relations)], dtype=np.uint32)
        assert g.kmpgpu_set_rules(gm._ctx, off.ctypes.data_as(u32p), t.ctypes.data_as(u32p), 1) == EINVAL      # no chains: the bound is n_pat + n_rel again
        # set_relations keeps the chains and drops the rules; the chains' terms move with the relations' count
        gm.set_chains(chains)
        gm.set_rules(rules)
        gm.set_relations(relations[:1])
        assert gm.chains == chains and gm.rules == []
        assert g.kmpgpu_scan_rules(gm._ctx, None, None, None, None, None) == ESTATE
        check_chains(gm, rows, counts)
        gm.set_rules([([gm.chain(2)], [gm.rel(0)])])
        check_rules(gm, np.concatenate([hits, rel_rows[:1], rows]), gm.rules, counts)
        gm.set_relations(relations)
        # launches: the chain kernel is one launch behind the scan launches, and a profile records it
        gm.profile_begin(64)
        pk = gm.scan_packets()
        n_pk = len(gm.profile_end(64))
        gm.profile_begin(64)
        chn = gm.scan_chains()
        n_ch = len(gm.profile_end(64))
        assert n_ch == n_pk + 1 and chn["timing"].launches == pk["timing"].launches == n_pk + 1
        gm.set_rules([([0], [])])
        gm.profile_begin(64)
        ru = gm.scan_rules()
        assert len(gm.profile_end(64)) == n_pk + 3 and ru["timing"].launches == n_pk + 3          # relation kernel, chain kernel, rules kernel
        gm.set_relations(None)
        gm.set_rules([([0], [])])
        gm.profile_begin(64)
        ru = gm.scan_rules()
        assert len(gm.profile_end(64)) == n_pk + 2 and ru["timing"].launches == n_pk + 2
        gm.set_chains(None)
        gm.set_rules([([0], [])])
        assert gm.scan_rules()["timing"].launches == n_pk + 1
        gm.set_chains(chains)
        # the general kernel does not mark: refused as kmpgpu_scan_packets refuses it
        gm.set_option(OPT_KERNEL, 1)
        assert g.kmpgpu_scan_chains(gm._ctx, None, None, None, None, None) == EINVAL
        gm.set_option(OPT_KERNEL, KERNEL_AUTO)
        # the context's counters stay untouched
        gm.set_option(OPT_ACCUMULATE, 1)
        gm.counts_reset()
        gm.scan_enqueue()
        check_chains(gm, rows, counts)
        assert gm.counts_read().tolist() == counts
        gm.set_option(OPT_ACCUMULATE, 0)
        # n_pkts == 0: zeros, nothing launched
        gm.load_arena(np.zeros(64, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.uint32))
        res = gm.scan_chains(hits=True)
        assert res["chain_pkt_counts"].tolist() == [0] * len(chains) and res["counts"].tolist() == [0] * n
        assert res["hits"].shape == (len(chains), 0) and res["timing"].launches == 0
        # set_patterns drops the chains
        gm.load_arena(K.HostArena.from_payloads(payloads))
        check_chains(gm, rows, counts)
        gm.set_patterns(pats)
        assert gm.chains == [] and gm.rules == [] and gm.relations == []
        assert g.kmpgpu_scan_chains(gm._ctx, None, None, None, None, None) == ESTATE
    finally:
        reset(gm)


# ------------------------------------------------------------------------------------------------
# 14. the fixture capture, loaded both ways
# ------------------------------------------------------------------------------------------------
def _fixture_chains(payloads, tokens):
    """three chains over tokens that co-occur in udp_1000.pcap, picked with the model: the triples with the most candidates, the first
    bounded so that it holds in some of its candidates and not in others"""
    st = MM.starts(payloads, tokens)
    hits = MM.hits(st)
    both = (hits[:, None, :] & hits[None, :, :]).sum(axis=2)
    np.fill_diagonal(both, 0)
    pairs = [divmod(int(i), len(tokens)) for i in np.argsort(-both, axis=None)[:30]]
    triples = []
    for a, b in pairs:
        third = (hits[a] & hits[b] & hits).sum(axis=1)
        third[[a, b]] = 0
        triples.append((a, b, int(np.argmax(third))))
    for a, b, c in triples:
        n_cand = int((hits[a] & hits[b] & hits[c]).sum())
        for span in (8, 32, 128, 512):
            first = (a, (b, -span, span), (c, -span, span))
            got = int(CM.chain_rows(st, tokens, [first])[0].sum())
            if 0 < got < n_cand:
                others = [t for t in triples if set(t) != {a, b, c}][:2]
                return [first, (others[0][0], (others[0][1], 0, 64), (others[0][2], None, None)), (others[1][2], (others[1][0], None, None), (others[1][1], None, -1))]
    raise AssertionError("no triple of tokens with hits and candidate misses")


@pytest.fixture(scope="module")
def capture(tokens):
    arena = K.HostArena.from_pcap(os.path.join(DATA, "udp_1000.pcap"), "udp")
    payloads = [bytes(arena.payload(k)) for k in range(arena.n_pkts)]
    chains = _fixture_chains(payloads, tokens)
    st = MM.starts(payloads, tokens)
    hits, rows = MM.hits(st), CM.chain_rows(st, tokens, chains)
    return arena, payloads, chains, hits, rows


def test_fixture_capture(gm, oracle, tokens, fixture_counts, capture):
    arena, payloads, chains, hits, rows = capture
    counts = fixture_counts["fixtures"]["udp_1000.pcap:udp"]["counts"]
    assert 0 < rows[0].sum() < candidates(hits, chains)[0].sum()
    try:
        reset(gm)
        gm.set_patterns(tokens)
        for how in ("arena", "frames"):
            if how == "arena":
                gm.load_arena(arena)
            else:
                assert gm.load_pcap_frames(os.path.join(DATA, "udp_1000.pcap"), "udp")[0] == len(payloads)
            gm.set_chains(chains)
            for _, kernel, fused in KERNELS:
                gm.set_option(OPT_KERNEL, kernel); gm.set_option(OPT_FUSED, fused)
                check_chains(gm, rows, counts)
            reset(gm)
    finally:
        reset(gm)


# ------------------------------------------------------------------------------------------------
# 15. the command lines: KMPGPU_CHAINS_FILE
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prog,extra", [("serial", []), ("openmp_data", ["1"]), ("openmp_data", ["3"])])
def test_cli_chains_file(tokens, tmp_path, capture, prog, extra):
    _, payloads, chains, hits, rows = capture
    n = len(tokens)

    def star(x):
        return "*" if x is None else str(x)

    cf = tmp_path / "chains.txt"
    cf.write_text("# p0 dmin dmax p1 ...\n\n" + "".join(str(ch[0]) + "".join(f" {star(lo)} {star(hi)} {p}" for p, lo, hi in ch[1:]) + "\n" for ch in chains))
    a0, b0 = chains[0][0], chains[0][1][0]
    relations = [(a0, b0, None, None)]
    lf = tmp_path / "relations.txt"
    lf.write_text(f"{a0} {b0} * *\n")
    al = tmp_path / "alerts.csv"
    with open(os.path.join(GOLDEN, "stdout_udp_1000_udp.txt")) as f:
        golden = f.read()
    rel_rows = MM.relation_rows(MM.starts(payloads, tokens), tokens, relations)
    for with_rel in (False, True):
        nr = 1 if with_rel else 0
        base = n + nr
        rules = [([a0, b0, base + 0], []), ([a0], [base + 0]), ([base + 1], []), ([], [base + 2, a0]), ([base + 0, base + 1], [])] + ([([n], [base])] if with_rel else [])

        def term(i):
            return str(i) if i < n else f"r{i - n}" if i < base else f"c{i - base}"

        rf = tmp_path / "rules.txt"
        rf.write_text("".join(" ".join([term(i) for i in pos] + ["!" + term(i) for i in neg]) + "\n" for pos, neg in rules))
        env = {"KMPGPU_CHAINS_FILE": str(cf), "KMPGPU_RULES_FILE": str(rf), "KMPGPU_ALERTS_FILE": str(al)}
        if with_rel:
            env["KMPGPU_RELATIONS_FILE"] = str(lf)
        r = run_cli(prog, extra=extra, env_extra=env)
        assert r.returncode == 0, r.stderr
        assert strip_elapsed(r.stdout) == golden
        got = [tuple(int(x) for x in line.split(",")) for line in al.read_text().splitlines()]
        want = MM.rule_rows(np.concatenate([hits] + ([rel_rows] if with_rel else []) + [rows]), rules)
        assert got == sorted((int(k), int(r_)) for r_, k in np.argwhere(want))
        assert want[0].any() and want[1].any()
    # (rf now names r0) a chains file that does not parse, a missing one, or the variable without its partners: exit 1 before any GPU work
    full = {"KMPGPU_RELATIONS_FILE": str(lf), "KMPGPU_RULES_FILE": str(rf), "KMPGPU_ALERTS_FILE": str(al)}
    bad = tmp_path / "bad.txt"
    bad.write_text("0 0 5 1\n0 9 3 1\n")
    r = run_cli(prog, extra=extra, env_extra=dict(full, KMPGPU_CHAINS_FILE=str(bad)))
    assert r.returncode == 1 and "line 2: " in r.stderr and r.stdout == ""
    r = run_cli(prog, extra=extra, env_extra=dict(full, KMPGPU_CHAINS_FILE=str(tmp_path / "none.txt")))
    assert r.returncode == 1 and r.stdout == ""
    r = run_cli(prog, extra=extra, env_extra={"KMPGPU_CHAINS_FILE": str(cf)})
    assert r.returncode == 1 and "KMPGPU_RULES_FILE" in r.stderr and r.stdout == ""
    r = run_cli(prog, extra=extra, env_extra={"KMPGPU_CHAINS_FILE": str(cf), "KMPGPU_RULES_FILE": str(rf)})
    assert r.returncode == 1 and "KMPGPU_ALERTS_FILE" in r.stderr and r.stdout == ""
    # without the chains the same rules file does not parse: c0 is no term
    r = run_cli(prog, extra=extra, env_extra=full)
    assert r.returncode == 1 and "line 1: " in r.stderr and r.stdout == ""
